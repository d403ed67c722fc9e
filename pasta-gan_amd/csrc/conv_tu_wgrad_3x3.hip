// Translation unit of the convolution family (conv_launch.h): the split weight-gradient kernel for 3x3 convolutions, every arithmetic and storage type.
#include "conv_launch.h"
#include "conv_wgrad_bf16x6.h"

namespace pasta {

void tu_wgrad3x3(int np, const WgradParams& p, int64_t blocks, hipStream_t s) {
    wgrad_arith_dispatch(np, p.io, [&](auto np_c, auto io_c) {
        constexpr int NP = decltype(np_c)::value, IO = decltype(io_c)::value;
        hipLaunchKernelGGL((conv_wgrad3x3_bf16x6_kernel<NP, IO>), dim3((unsigned)blocks), dim3(256), Wgrad3x3Tile::lds_bytes(Arith<NP>::npw), s, p);
    });
}
}  // namespace pasta
