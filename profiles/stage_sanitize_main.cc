// A stand-alone run of the stage driver for the host sanitizers (profiles/stage_sanitize.sh): generate_many over the given
// bucket BEDs through the test provider and the scalar oracle (oracle/extz2_oracle.c), no device and no Python in the process.
//   stage_sanitize GENOME.fa BUCKET.bed [BUCKET.bed ...]      (SDF_LANES, SDF_BUCKET_LANES, SDF_HOST_THREADS as the CLI reads them)
#include <cstdio>
#include <string>
#include <vector>

#include "../oracle/extz2_oracle.h"
#include "../sedef_amd/csrc/host/sedef_host.h"

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  try {
    sdfh::set_stage_settings(sdfh::StageSettings::from_env());
    const auto dp = sdfh::make_test_provider((sdfh::test_dp_fn)sdfo_extz2);
    const std::vector<std::string> beds(argv + 2, argv + argc);
    long lines = 0, hits = 0;
    for (const auto &st : sdfh::generate_many(argv[1], beds, 11, sdfh::Params(), *dp, ".aligned.bed", "", stderr))
      lines += st.lines, hits += st.total_written;
    printf("%zu buckets, %ld lines, %ld hits\n", beds.size(), lines, hits);
    return hits > 0 ? 0 : 1;
  } catch (std::string &s) {
    fprintf(stderr, "failed: %s\n", s.c_str());
    return 1;
  }
}
