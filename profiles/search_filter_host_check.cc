// Stand-alone host program for sanitizer runs of sdf_search_filter_host and sdf_search_filter_tasks_host (no GPU is touched, no
// python is involved).  Build and run from the repository root:
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Iinclude -Isedef_amd/csrc \
//         -x hip profiles/search_filter_host_check.cc sedef_amd/csrc/search_host.hip -o /tmp/search_filter_host_check
// (search_host.hip holds the search family's host forms and needs no kernel source beside it)
//   python tests/golden/make_golden_search_filter.py --dump-cases /tmp/cases.bin
//   /tmp/search_filter_host_check /tmp/cases.bin
// cases.bin holds fixture cases back to back, little endian: u64 pool_bytes, the pool, u64 n, n sdf_filter_task, one
// sdf_filter_params, n sdf_filter_rec (the records expected).  The pool and the arrays are copied into heap blocks of their exact
// size, so a read one byte outside them is an error the sanitizer reports.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sedef_hip.h"

template <class T>
static T *exact(const std::vector<char> &file, size_t &at, size_t n) {
  T *p = (T *)malloc(n * sizeof(T) + (n ? 0 : 1));
  memcpy(p, file.data() + at, n * sizeof(T));
  at += n * sizeof(T);
  return p;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<char> file;
  char buf[65536];
  for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) file.insert(file.end(), buf, buf + k);
  fclose(f);
  size_t at = 0, cases = 0, records = 0;
  while (at < file.size()) {
    uint64_t pool_bytes, n;
    memcpy(&pool_bytes, file.data() + at, 8), at += 8;
    char *pool = exact<char>(file, at, pool_bytes);
    memcpy(&n, file.data() + at, 8), at += 8;
    sdf_filter_task *tasks = exact<sdf_filter_task>(file, at, n);
    sdf_filter_params *P = exact<sdf_filter_params>(file, at, 1);
    sdf_filter_rec *want = exact<sdf_filter_rec>(file, at, n), *got = (sdf_filter_rec *)malloc(n * sizeof *got + 1);
    if (sdf_search_filter_host(pool, pool_bytes, P, tasks, n, got) != SDF_OK || memcmp(got, want, n * sizeof *got)) return 1;
    // a refused call writes nothing
    if (n) {
      tasks[n - 1].q_off = (int64_t)pool_bytes, tasks[n - 1].q_len = 1;
      memset(got, 0x55, n * sizeof *got);
      if (sdf_search_filter_host(pool, pool_bytes, P, tasks, n, got) != SDF_ERR_INVALID || ((unsigned char *)got)[0] != 0x55) return 1;
    }
    free(pool), free(tasks), free(P), free(want), free(got);
    ++cases, records += n;
  }
  // the task builder on arrays of its own: three windows, seven intervals, both strands, both values of allow_extend
  const sdf_minimizer q[3] = {{5, 10, 0, 0}, {6, 40, 0, 0}, {7, 90, 0, 0}};
  const sdf_search_window windows[3] = {{1, 1, 0, 0, 0}, {1, 1, 0, 0, SDF_SEARCH_NOLIMIT}, {1, 1, 0, 0, 0}};
  const uint64_t first[4] = {0, 4, 5, 7};
  const sdf_search_interval iv[7] = {{100, 130}, {100, 130}, {100, 130}, {100, 130}, {0, 9}, {280, 300}, {250, 400}};
  const sdf_search_roll_rec rolls[7] = {{110, 130, 0, 0, 3, 0}, {110, 130, 0, 0, -1, 0}, {0, 0, 0, 0, 0, SDF_ROLL_WIDE}, {110, 130, 0, 0, 2, SDF_ROLL_WIDE},
                                        {0, 20, 0, 0, 1, 0},    {280, 300, 0, 0, 0, 0},  {260, 280, 0, 0, 5, SDF_ROLL_BADWINDOW}};
  size_t live = 0;
  for (int v = 0; v < 8; v++) {
    sdf_filter_task *out = (sdf_filter_task *)malloc(7 * sizeof *out);
    if (sdf_search_filter_tasks_host(q, 3, windows, first, iv, rolls, 110, 300, 20, 1000, v & 1, 5000, v & 2, v & 4, out) != SDF_OK) return 1;
    for (int t = 0; t < 7; t++) live += !(out[t].flags & SDF_FILTER_SKIP);
    free(out);
  }
  printf("search_filter_host_check: %zu cases, %zu records equal; task builder %zu live tasks of 56\n", cases, records, live);
  return live == 24 ? 0 : 1;
}
