// dd_gemm2_kernel, the conv instantiations (gemm2_kernel.h)
#include "gemm2_kernel.h"

int ddg::launch_gemm2_conv(int dtype, unsigned form, const GemmParams& p, const Plan& pl, hipStream_t s) {
  return dispatch<Gemm2, F_CONV>(dtype, form, p, pl, s);
}
