#!/bin/bash
# Tools-only build of the library with -DLSL_EXPERIMENTS: timing probes (LSL_PROBE: results WRONG on purpose), the rejected GEMM
# structures (tools/experiments/k_gemm_pp, k_gemm_drain, variants 13 / 20-22 / 30), the scalar output head and every LSL_* tuning knob.
# The product library (lam_slide_amd/liblamslide_hip.so, built by __graft_entry__.build()) contains none of this.
# The same translation units and per-unit options as the product (lam_slide_amd/_lib.py UNITS), compiled side by side.
set -eu
root=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$root/tools/_exp/obj"
objs=()
while read -r unit flags; do
  obj="$root/tools/_exp/obj/${unit%.hip}.o"
  /opt/rocm/bin/hipcc $flags -DLSL_EXPERIMENTS -I"$root/tools/experiments" -I"$root/lam_slide_amd/csrc" -c "$root/lam_slide_amd/csrc/$unit" -o "$obj" &
  objs+=("$obj")
done < <(cd "$root" && python3 -c "
from lam_slide_amd import _lib
for name, extra in _lib.UNITS: print(name, *[f for f in _lib.BASE_FLAGS if f != '-fvisibility=hidden'], *extra)")
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$root/tools/_exp/liblamslide_hip_exp.so" "${objs[@]}"
echo "built $root/tools/_exp/liblamslide_hip_exp.so"
