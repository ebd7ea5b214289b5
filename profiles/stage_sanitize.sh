#!/bin/bash
# AddressSanitizer + UndefinedBehaviorSanitizer, then ThreadSanitizer, over the stage driver as a stand-alone program
# (profiles/stage_sanitize_main.cc: generate_many through the test provider and the scalar oracle; no device, no Python in
# the process): every host source of sedef_amd/host.py: _SOURCES, the oracle and the program compiled with the sanitizer.
# Input: the genome of tests/test_host_pipeline.py: test_generate_stage_cpu_hook (tests/hostgen.py, seed 1), its bucket three
# times.  Two runs per sanitizer: the buckets two at a time (SDF_BUCKET_LANES, the default), and two lanes of super-batches
# inside every bucket (SDF_LANES=2, SDF_SUPER_BATCH=2).  Needs sedef_amd/lib/libsedef_hip.so (the GPU provider's symbols are
# linked, never called).  Run where the project is built, no GPU needed: bash profiles/stage_sanitize.sh
# After the split of the stage driver into files by job: 4 runs of 3 buckets (18 lines, 15 hits each), no report.
cd "$(dirname "$0")/.." || exit 1
SRCS=$(python3 -c "import sedef_amd.host as h; print(' '.join(h.HOST_SRC + '/' + f for f in h._SOURCES))")
W=$(mktemp -d)
python3 -c "import sys; sys.path.insert(0, 'tests'); import hostgen; hostgen.make_genome('$W/genome.fa', seed=1)" || exit 1
for b in a b c; do cp $W/genome.fa.bed $W/bucket_$b.bed; done
rc=0
for san in address,undefined thread; do
  gcc -O1 -g -fsanitize=$san -fno-omit-frame-pointer -c oracle/extz2_oracle.c -o $W/oracle.o || exit 1
  g++ -O1 -g -fsanitize=$san -fno-omit-frame-pointer -std=c++17 -Wall -o $W/stage_sanitize profiles/stage_sanitize_main.cc \
      $SRCS $W/oracle.o -Lsedef_amd/lib -lsedef_hip -lpthread -Wl,-rpath,$PWD/sedef_amd/lib || exit 1
  export ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 TSAN_OPTIONS=halt_on_error=0:exitcode=66
  echo "== -fsanitize=$san: buckets two at a time"
  SDF_HOST_THREADS=4 $W/stage_sanitize $W/genome.fa $W/bucket_a.bed $W/bucket_b.bed $W/bucket_c.bed 2> $W/log.$san.1 || rc=1
  echo "== -fsanitize=$san: SDF_LANES=2"
  SDF_HOST_THREADS=4 SDF_LANES=2 SDF_SUPER_BATCH=2 $W/stage_sanitize $W/genome.fa $W/bucket_a.bed $W/bucket_b.bed $W/bucket_c.bed 2> $W/log.$san.2 || rc=1
  grep -l "Sanitizer\|runtime error" $W/log.$san.* && { rc=1; cat $W/log.$san.*; }
  cmp $W/bucket_a.bed.aligned.bed $W/bucket_c.bed.aligned.bed || rc=1
done
[ $rc = 0 ] && echo "no sanitizer report" || echo "sanitizer reports or failures above (logs in $W)"
exit $rc
