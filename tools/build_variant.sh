#!/bin/bash
# tools/build_variant.sh <name> [-D...]: build ab/libmoonrt_<name>.so with extra defines (A/B experiments only)
#   trialwide  -DMRTX_TRIAL_WIDE=1 [-DMRTX_TRIAL_WIDE_K=0..3] [-DMRTX_TRIAL_WIDE_MIN=0..] [-DMRTX_RENDER_SGPRS=96]
#              the trial segment's steps dealt out over the wave (measured slower, ships as 0)
#   proftrial  -DMRTX_PROF -DMRTX_PROF_TRIAL     the trial's wave-level counts for tools/prof_sections.py (TRIAL=1 PATH_SEG=2,4)
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1; shift
mkdir -p "$ROOT/ab"
cd "$ROOT/moonrtx_amd/csrc"
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -shared --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -fno-slp-vectorize \
  -fhip-fp32-correctly-rounded-divide-sqrt "$@" mrtx_kernels.hip mrtx_terrain.hip mrtx_traverse.hip mrtx_relief.hip mrtx_api.hip -o "$ROOT/ab/libmoonrt_$NAME.so"
echo "built ab/libmoonrt_$NAME.so"
