#!/bin/bash
# VGPR / scratch / occupancy of every kernel whose mangled name matches $1 (default k_gemm_glds), over the translation units of the library,
# each compiled with its own options (lam_slide_amd/_lib.py: BASE_FLAGS + UNITS; REGS_FLAGS adds options to every unit)
root=$(cd "$(dirname "$0")/.." && pwd)
cd "$root" && python3 -c "
from lam_slide_amd import _lib
for name, extra in _lib.UNITS: print(name, *_lib.BASE_FLAGS, *extra)" | while read -r unit flags; do
  /opt/rocm/bin/hipcc $flags ${REGS_FLAGS:-} --cuda-device-only -S -o /dev/null "$root/lam_slide_amd/csrc/$unit" -Rpass-analysis=kernel-resource-usage 2>&1
done | grep -E "Function Name|VGPRs:|AGPRs|ScratchSize|Occupancy|SGPRs:" | grep -A5 "${1:-k_gemm_glds}" | sed 's/.*Function Name: /K /; s/.*remark: *//; s/\[-Rpass.*//' | grep -v "^--" | paste - - - - - - | sed 's/  */ /g; s/TotalSGPRs/S/; s/ScratchSize \[bytes\/lane\]/scratch/; s/Occupancy \[waves\/SIMD\]/occ/; s/AGPRs: 0//' | cut -c1-300
