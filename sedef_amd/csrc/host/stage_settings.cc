// The stage driver's own settings: read from the environment in one place, kept for the run (sedef_host.h: StageSettings).
#include <cstdlib>
#include <mutex>

#include "sedef_host.h"

namespace sdfh {

StageSettings StageSettings::from_env() {
  StageSettings s;
  auto num = [](const char *name, long lo, long hi, long dflt) {
    const char *e = getenv(name);
    if (!e || !*e) return dflt;
    char *end = nullptr;
    const long v = strtol(e, &end, 10);
    if (end == e || *end) throw std::string(name) + "=" + e + ": not a number";
    if (v < lo || v > hi) throw std::string(name) + "=" + e + ": out of range";
    return v;
  };
  s.device = (int)num("SDF_DEVICE", 0, 1023, 0);
  s.lanes = (int)num("SDF_LANES", 0, 8, 0);
  s.super_batch = (int)num("SDF_SUPER_BATCH", 0, 1 << 30, 0);
  s.gpu_anchors = num("SDF_GPU_ANCHORS", 0, 1, 1) != 0;
  s.host_threads = (int)num("SDF_HOST_THREADS", 0, 4096, 0);
  if (const char *e = getenv("SDF_STAGE_WS_GIB")) s.stage_ws_gib = atof(e) > 0 ? atof(e) : 0;
  s.debug_timing = getenv("SDF_DEBUG_TIMING") != nullptr;
  s.resident_dp = num("SDF_RESIDENT_DP", 0, 1, 1) != 0;
  s.anchor_parts = (int)num("SDF_ANCHOR_PARTS", 0, 16, 0);
  s.bucket_lanes = (int)num("SDF_BUCKET_LANES", 1, 4, 2);
  s.translate_limit = (int)num("SDF_TEST_TRANSLATE_LIMIT", 1, 0x7fffffff, 100 * 1000 * 1000);
  s.stats_resident = num("SDF_STATS_RESIDENT", 0, 1, 0) != 0;
  s.stats_cuts_device = num("SDF_STATS_CUTS_DEVICE", 0, 1, 0) != 0;
  s.bucket_device = num("SDF_BUCKET_DEVICE", 0, 1, 0) != 0;
  s.stats_diff_host = num("SDF_STATS_DIFF_HOST", 0, 1, 0) != 0;
  s.stats_recall_host = num("SDF_STATS_RECALL_HOST", 0, 1, 0) != 0;
  s.report_host = num("SDF_REPORT_HOST", 0, 1, 0) != 0;
  s.stats_recall_ignore_strand = num("SDF_STATS_RECALL_IGNORE_STRAND", 0, 1, 0) != 0;
  s.search_wide = (int)num("SDF_SEARCH_WIDE_DEVICE", 0, 1 << 20, 0);
  s.search_lanes = (int)num("SDF_SEARCH_LANES", 1, 16, 1);
  s.stage_resident = num("SDF_STAGE_RESIDENT", 0, 1, 0) != 0;
  s.fetch_device = num("SDF_STAGE_FETCH_DEVICE", 0, 1, 0) != 0;
  if (const char *e = getenv("SDF_DEVICES"))
    for (const char *c = e; *c;) {
      char *end = nullptr;
      const long d = strtol(c, &end, 10);
      if (end == c) throw std::string("SDF_DEVICES=") + e + ": a list of device ordinals";
      s.devices.push_back((int)d);
      c = *end == ',' ? end + 1 : end;
    }
  return s;
}
namespace {
StageSettings g_stage_settings;
std::mutex g_stage_settings_mu;
}  // namespace
const StageSettings &stage_settings() { return g_stage_settings; }
void set_stage_settings(const StageSettings &s) {
  std::lock_guard<std::mutex> g(g_stage_settings_mu);
  g_stage_settings = s;
}

}  // namespace sdfh
