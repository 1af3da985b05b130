// compile-only harness for conv3_wino4.h (register / spill / ISA inspection in seconds instead of the time all of conv3.hip takes):
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=fast -I include -I <csrc> -c scripts/dbg/wino4_standalone.hip -o /tmp/w4.o -save-temps
#include "common.h"
namespace {
template <int V> struct wino_const { static constexpr int value = V; };
#include "conv3_wino4.h"
}
void wino4_standalone_launch(Wino4Args p, hipStream_t st) {
    hipLaunchKernelGGL(conv3_wino4_kernel<false>, dim3(1), dim3(W4_THREADS), 0, st, p);
    hipLaunchKernelGGL(conv3_wino4_kernel<true>, dim3(1), dim3(W4_THREADS), 0, st, p);
}
