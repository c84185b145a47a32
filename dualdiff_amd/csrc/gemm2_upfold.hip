// dd_gemm2u_kernel, the folded-upsample conv form of dd_gemm2_kernel (gemm2_kernel.h)
#include "gemm2_kernel.h"

int ddg::launch_gemm2_upfold(int dtype, unsigned form, const GemmParams& p, const Plan& pl, hipStream_t s) {
  return dispatch<Gemm2U, F_UPFOLD>(dtype, form, p, pl, s);
}
