#!/bin/sh
# Build (if needed) and run the MFMA rate probe; the output belongs in profiles/fp16_mfma_probe.txt.
set -e
here="$(cd "$(dirname "$0")" && pwd)"
if [ ! -x "$here/mfma_f16_vs_bf16" ] || [ "$here/mfma_f16_vs_bf16.hip" -nt "$here/mfma_f16_vs_bf16" ]; then
  "${HIPCC:-/opt/rocm/bin/hipcc}" --offload-arch=gfx950 -O3 -o "$here/mfma_f16_vs_bf16" "$here/mfma_f16_vs_bf16.hip"
fi
exec "$here/mfma_f16_vs_bf16"
