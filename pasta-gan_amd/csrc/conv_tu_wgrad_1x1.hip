// Translation unit of the convolution family (conv_launch.h): the split weight-gradient kernel for 1x1 convolutions, every arithmetic and storage type.
#include "conv_launch.h"
#include "conv_wgrad_bf16x6.h"

namespace pasta {

void tu_wgrad1x1(int np, int WA, const WgradParams& p, int64_t blocks, hipStream_t s) {
    wgrad_arith_dispatch(np, p.io, [&](auto np_c, auto io_c) {
        constexpr int NP = decltype(np_c)::value, IO = decltype(io_c)::value, NPW = Arith<NP>::npw;
        const size_t lds = WA == 2 ? Wgrad1x1Tile<2, 2>::lds_bytes(NPW) : Wgrad1x1Tile<1, 1>::lds_bytes(NPW);
        if (WA == 2) hipLaunchKernelGGL((conv_wgrad1x1_bf16x6_kernel<2, 2, NP, IO>), dim3((unsigned)blocks), dim3(256), lds, s, p);
        else         hipLaunchKernelGGL((conv_wgrad1x1_bf16x6_kernel<1, 1, NP, IO>), dim3((unsigned)blocks), dim3(256), lds, s, p);
    });
}
}  // namespace pasta
