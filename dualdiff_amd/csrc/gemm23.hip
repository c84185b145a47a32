// dd_gemm2_kernel, the dense instantiations (gemm2_kernel.h), and the dd_gemm3_kernel family (gemm3_kernel.h).
//
// One translation unit for both on purpose.  The 32-row tiles of the two families share one instantiation of the general
// epilogue, store_tile<T, 1, 2, false>, and dd_gemm3_kernel calls it with constant (absent) LayerNorm-fold arguments: compiled
// without dd_gemm2_kernel's call next to it, interprocedural constant propagation specialises that epilogue before it is
// inlined, and the four 32x64/p4 and /p6 kernels come out 20 bytes longer than the ones every measurement of this project
// was taken with (tools/kernel_identity.py shows it).
#include "gemm2_kernel.h"
#include "gemm3_kernel.h"

int ddg::launch_gemm2_dense(int dtype, unsigned form, const GemmParams& p, const Plan& pl, hipStream_t s) {
  return dispatch<Gemm2, F_DENSE>(dtype, form, p, pl, s);
}
int ddg::launch_gemm3(int dtype, unsigned form, const GemmParams& p, const Plan& pl, hipStream_t s) {
  return dispatch<Gemm3, F_DENSE, F_GEGLU>(dtype, form, p, pl, s);
}
