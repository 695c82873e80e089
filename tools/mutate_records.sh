#!/bin/bash
# Mutation check of tests/test_gpu_hostile_records.py: build copies of libptrace_surface.so and libptrace_scatter.so with the
# handling of a caller's record made WRONG in ways a careless edit could, then run the hostile-record tests on each.  Every
# mutant must fail a named test (profiles/hostile_records_gpu_tests.log records which).
# Only mutants that keep every address inside the textures and the record table: NO mutant removes a clamp or a slot check.
# usage (repository root; the second half on the GPU box): tools/mutate_records.sh build [names] | run [names]
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$ROOT/build_variants
mkdir -p $OUT
ONLY=" ${*:2} "  # build / run these mutants only (default: all)
MUTANTS="fmax fmod texel roulette"
if [ "$1" = "run" ] && [ $# -gt 1 ]; then MUTANTS="${*:2}"; fi
mutate() {  # name, file of csrc/, sed expression
  local name=$1 file=$2 expr=$3
  if [ "$ONLY" != "  " ] && [[ "$ONLY" != *" $name "* ]]; then return 0; fi
  local tmp=$(mktemp -d)
  mkdir -p $tmp/pytracer_amd $tmp/include   # (the sources include ../../include/ptrace.h: keep that shape)
  cp -r $ROOT/pytracer_amd/csrc $tmp/pytracer_amd/csrc
  cp $ROOT/include/*.h $tmp/include/
  for f in $file; do
    sed -i "$expr" $tmp/pytracer_amd/csrc/$f
    if cmp -s $tmp/pytracer_amd/csrc/$f $ROOT/pytracer_amd/csrc/$f; then echo "mutant $name: the edit did not apply to $f"; exit 1; fi
  done
  for lib in surface scatter; do
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-fast-math -std=c++17 -fPIC -shared -Wno-unused-function \
        -Wno-pass-failed -o $OUT/libptrace_${lib}_rmut_$name.so $tmp/pytracer_amd/csrc/ptrace_$lib.hip
  done
  rm -rf $tmp
  echo "built $name"
}
if [ "$1" = "build" ]; then
  # 1: max2 as fmax -- a NaN operand is dropped instead of following Python's max(a, b)
  # 2: the checkered parity by fmod's sign -- negative odd cells come out even (C's remainder takes the dividend's sign)
  # 3: a negative or NaN texel product goes to the LAST column / row instead of the first (still inside the texture)
  # 4: the roulette's draw > q as draw >= q -- a draw EQUAL to q survives, and q = 1 then forms 1 / 0
  mutate fmax pt_math.h 's|PT_DEV double max2(double a, double b) { return (b > a) ? b : a; }|PT_DEV double max2(double a, double b) { return fmax(a, b); }|'
  mutate fmod pt_shade.h 's|const bool odd_u = floor(tu \* 0.5) \* 2.0 != tu, odd_v = floor(tv \* 0.5) \* 2.0 != tv;|const bool odd_u = fmod(tu, 2.0) > 0.0, odd_v = fmod(tv, 2.0) > 0.0;|'
  mutate texel "pt_surface.h pt_scatter.h" 's|if (!(f >= 0.0)) return 0;|if (!(f >= 0.0)) return (long long)w - 1;|'
  mutate roulette pt_scatter.h 's|if (pcg_float(g) > q) {|if (pcg_float(g) >= q) {|'
  exit 0
fi
cd $ROOT
run() {  # one pytest step; 0 and 1 (tests failed: what a mutant is for) go on, anything else (a fault, an abort, a time limit) ends the run
  local rc
  set +e
  "$@" 2>&1 | grep -E "^(FAILED|ERROR)|passed|failed" | cut -c1-220
  rc=${PIPESTATUS[0]}
  set -e
  if [ $rc -gt 1 ]; then echo "exit status $rc: stopping"; exit $rc; fi
}
for m in $MUTANTS; do
  echo "== mutant $m"
  export PTRACE_SURFACE_LIB=$OUT/libptrace_surface_rmut_$m.so PTRACE_SCATTER_LIB=$OUT/libptrace_scatter_rmut_$m.so
  run timeout -k 10 300 python -m pytest tests/test_gpu_hostile_records.py -q -rf -p no:cacheprovider
done
