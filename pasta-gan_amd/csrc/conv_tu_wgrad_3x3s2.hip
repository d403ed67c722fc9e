// Translation unit of the convolution family (conv_launch.h): the split weight-gradient kernel for 3x3s2 convolutions, every arithmetic and storage type.
#include "conv_launch.h"
#include "conv_wgrad_bf16x6.h"

namespace pasta {

void tu_wgrad3x3s2(int np, const WgradParams& p, int64_t blocks, hipStream_t s) {
    if (p.l_pieces) {       // L as the producer wrote it (pieces.hip): copies and transposed LDS reads, no split (the planner checked: F16X3, pad 0, one group)
        hipLaunchKernelGGL((conv_wgrad3x3s2_pieces_kernel<0>), dim3((unsigned)blocks), dim3(256), 0, s, p);
        return;
    }
    wgrad_arith_dispatch(np, p.io, [&](auto np_c, auto io_c) {
        constexpr int NP = decltype(np_c)::value, IO = decltype(io_c)::value;
        const size_t lds = Wgrad3x3s2Tile::lds_bytes(Arith<NP>::npw);
        if (p.pad_w == 1) hipLaunchKernelGGL((conv_wgrad3x3s2_bf16x6_kernel<1, NP, IO>), dim3((unsigned)blocks), dim3(256), lds, s, p);
        else              hipLaunchKernelGGL((conv_wgrad3x3s2_bf16x6_kernel<0, NP, IO>), dim3((unsigned)blocks), dim3(256), lds, s, p);
    });
}
}  // namespace pasta
