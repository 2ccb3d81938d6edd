#!/bin/bash
# AddressSanitizer + UBSan build of the host code behind the encoder leaders' optimiser, update and population entries, as ONE
# stand-alone program with tools/asan/update_seam_driver.cpp's main (the sanitizers' runtime is linked into the program: nothing
# is preloaded, nothing is loaded into Python).  The device code is compiled as it is (-fno-gpu-sanitize) and never runs: the
# driver needs no device.
#   bash tools/asan_update_seam.sh   -> prints "update seam driver: ok", exit 0; any ASan/UBSan report fails the run
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${TMPDIR:-/tmp}/evac_asan_update_seam
mkdir -p "$OUT"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
C="$ROOT/evacuation_amd/csrc"
$HIPCC -O1 -g --offload-arch=gfx950 -ffp-contract=off -std=c++17 -Xarch_host -fsanitize=address,undefined -fno-gpu-sanitize \
  -Xarch_host -fno-sanitize-recover=undefined -I"$ROOT/include" \
  "$C/evac_api.hip" "$C/evac_train_api.hip" "$C/evac_population_api.hip" "$C/evac_deepsets_train_api.hip" \
  "$C/evac_transformer_train_api.hip" "$C/evac_deepsets_update_api.hip" \
  "$C/evac_transformer_update_api.hip" "$C/evac_deepsets_population_api.hip" "$C/evac_deepsets_population_evaluate_api.hip" \
  "$C/evac_transformer_population_api.hip" "$C/evac_transformer_population_evaluate_api.hip" \
  "$C/evac_transformer_population_update_api.hip" "$ROOT/tools/asan/update_seam_driver.cpp" -o "$OUT/update_seam_driver"
ASAN_OPTIONS=detect_leaks=1:halt_on_error=1:abort_on_error=0 "$OUT/update_seam_driver"
