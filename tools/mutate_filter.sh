#!/bin/bash
# Mutation check of the scattered-ray filter's tests: build copies of the library with the filter made WRONG in ways a
# careless edit could, then run tests/test_gpu_probes.py (filtered against exhaustive query), the aimed rays of
# tests/test_gpu_aimed_rays.py (the same query against the CPU oracle) and the random scenes on each.
# Every mutant must fail somewhere; noeps and noE are the known survivors (profiles/aimed_rays_mutants.log says why).
# usage (repository root; the second half on the GPU box): tools/mutate_filter.sh build [names] | run [names]
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$ROOT/build_variants
mkdir -p $OUT
ONLY=" ${*:2} "  # build / run these mutants only (default: all)
MUTANTS="r98 slack halfseg behind shortseg noeps nofar noE gersh"
if [ "$1" = "run" ] && [ $# -gt 1 ]; then MUTANTS="${*:2}"; fi
mutate() {  # name, sed expression applied to pt_query.h / pt_scene_build.h
  local name=$1 file=$2 expr=$3
  if [ "$ONLY" != "  " ] && [[ "$ONLY" != *" $name "* ]]; then return 0; fi
  local tmp=$(mktemp -d)
  mkdir -p $tmp/pytracer_amd $tmp/include   # (the sources include ../../include/ptrace.h: keep that shape)
  cp -r $ROOT/pytracer_amd/csrc $tmp/pytracer_amd/csrc
  cp $ROOT/include/*.h $tmp/include/
  sed -i "$expr" $tmp/pytracer_amd/csrc/$file
  if cmp -s $tmp/pytracer_amd/csrc/$file $ROOT/pytracer_amd/csrc/$file; then echo "mutant $name: the edit did not apply"; exit 1; fi
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-fast-math -std=c++17 -fPIC -shared -Wno-unused-function \
      -Wno-pass-failed -o $OUT/libptrace_fmut_$name.so $tmp/pytracer_amd/csrc/ptrace.hip
  rm -rf $tmp
  echo "built $name"
}
if [ "$1" = "build" ]; then
  # 1: radii 2 % too small in the tables           2: the margin for the rounding of o dropped AND the slack inverted
  # 3: shadow rays clamped to half the segment      4: balls behind the origin "seen" through the wrong sign of the clamp
  mutate r98 pt_scene_build.h 's|(double)\*r \* (double)\*r \* (1.0 + 8.1e-6)|(double)*r * (double)*r * 0.96|'
  mutate slack pt_query.h 's|__builtin_amdgcn_rsqf(dd) \* 1.0000041f|__builtin_amdgcn_rsqf(dd) * 0.9995f|'
  mutate halfseg pt_query.h 's|const float tlen = ANYHIT ? (float)tmax \* (dd \* rn) \* (1.0f + 1e-5f) : 0.0f;|const float tlen = ANYHIT ? 0.5f * (float)tmax * (dd * rn) : 0.0f;|'
  mutate behind pt_query.h 's|__builtin_fmaxf(vd.x, 0.0f), __builtin_fmaxf(vd.y, 0.0f)|__builtin_fminf(vd.x, 0.0f), __builtin_fminf(vd.y, 0.0f)|'
  # 5: the segment's end 1e-4 short instead of 1e-5 long     6: spheres entered into the grid's cells without the margin eps
  # 7: no ray is "far": origins beyond 100 x the grid's coordinates walk the grid on their fp32 copy too
  # 8: no allowance for the rounding of the origin to fp32    9: a sphere's radius from the diagonal of M^T M alone (exact only
  #    without shear)
  mutate shortseg pt_query.h 's|const float tlen = ANYHIT ? (float)tmax \* (dd \* rn) \* (1.0f + 1e-5f) : 0.0f;|const float tlen = ANYHIT ? (float)tmax * (dd * rn) * (1.0f - 1e-4f) : 0.0f;|'
  mutate noeps pt_scene_build.h 's|const double eps = 2e-3 \* s.grid_cell\[q\] + 1e-4 \* cmax, c = ball(k, q)|const double eps = 0.0, c = ball(k, q)|'
  mutate nofar pt_scene_build.h 's|s.grid_far_eo = (float)(1e-4 \* cmax);|s.grid_far_eo = 1e30f;|'
  mutate noE pt_query.h 's|const float e7 = 2e-7f \* omax;|const float e7 = 0.0f;|'
  mutate gersh pt_scene_build.h 's|lam = std::max(lam, std::fabs(A\[i\]\[0\]) + std::fabs(A\[i\]\[1\]) + std::fabs(A\[i\]\[2\]));|lam = std::max(lam, std::fabs(A[i][i]));|'
  exit 0
fi
cd $ROOT
run() {  # one pytest step; 0 and 1 (tests failed: what a mutant is for) go on, anything else (a fault, an abort, a time limit) ends the run
  local rc
  set +e
  "$@" 2>&1 | tail -1
  rc=${PIPESTATUS[0]}
  set -e
  if [ $rc -gt 1 ]; then echo "exit status $rc: stopping"; exit $rc; fi
}
for m in $MUTANTS; do
  echo "== mutant $m"
  export PTRACE_LIB=$OUT/libptrace_fmut_$m.so
  run timeout -k 10 300 python -m pytest tests/test_gpu_probes.py -q -k "filtered_query"
  run timeout -k 10 300 python -m pytest tests/test_gpu_aimed_rays.py -q -k lanes
  PT_FUZZ_SEEDS=40 run timeout -k 10 300 python -m pytest tests/test_gpu_parity.py -q -x -k "random_scenes or c4 or c3_pathtracer"
done
unset PTRACE_LIB
echo "== the library as shipped"
run timeout -k 10 300 python -m pytest tests/test_gpu_probes.py -q -k "filtered_query"
run timeout -k 10 300 python -m pytest tests/test_gpu_aimed_rays.py -q -k lanes
