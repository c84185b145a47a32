#!/bin/bash
# Diagnostic builds of the C-ABI library (NOT the product): libdd_nomfma.so drops the matrix instructions of the fp16
# GEMM main loops, libdd_nodma.so the LDS-DMA loads; load one with DD_HIP_LIB=... to see which side bounds a kernel.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
L=$R/dualdiff_amd/lib
python3 -c "import sys; sys.path.insert(0, '$R'); from dualdiff_amd import _build; _build.build_native()"
GEMM="gemm1 gemm23 gemm2_geglu gemm2_conv gemm2_upfold gemm4 conv3s"      # the GEMM / conv kernel families' translation units
for V in NOMFMA NODMA; do
  v=$(echo $V | tr A-Z a-z)
  for S in $GEMM; do
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-value -DNDEBUG -DDD_DBG_$V \
      -c $R/dualdiff_amd/csrc/$S.hip -o /tmp/${S}_$v.o &
  done
done
wait
REST=$(ls $L/obj/*.o | grep -v -E "/($(echo $GEMM | tr ' ' '|'))\.o")
for v in nomfma nodma; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $L/libdd_$v.so $(for S in $GEMM; do echo /tmp/${S}_$v.o; done) $REST
done
# attention: matrix instructions removed / exponentials replaced by moves (tools/attn_sides.py)
for V in NOMFMA NOEXP NOSTAGE; do
  v=$(echo $V | tr A-Z a-z)
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-value -DNDEBUG -mllvm -amdgpu-mfma-vgpr-form=1 \
    -fno-honor-nans -DDD_DBG_$V -c $R/dualdiff_amd/csrc/attention.hip -o /tmp/attn_$v.o &
done
wait
for v in nomfma noexp nostage; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $L/libdd_attn_$v.so /tmp/attn_$v.o $(ls $L/obj/*.o | grep -v "/attention.o")
done
ls -la $L/*.so
