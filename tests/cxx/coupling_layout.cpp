// The layout of the SHOC and the P3 coupling workspaces (pam_amd/csrc/coupling_workspace.h) without a GPU: the carve function under both
// zero-size policies and the two tables, against the closed formulas of include/pam_amd_modules.h that the GPU tests assert on
// workspace_bytes.  Built with -fsanitize=address,undefined by tests/test_coupling_layout.py; exit status 0 = every check held.
#include <cstdio>
#include <vector>

#include "../../pam_amd/csrc/coupling_workspace.h"

namespace cw = pama::coupling;

static int failures = 0;
#define CHECK(cond, ...)                                       \
  do {                                                         \
    if (!(cond)) {                                             \
      failures++;                                              \
      std::fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
      std::fprintf(stderr, __VA_ARGS__);                       \
      std::fprintf(stderr, "\n");                              \
    }                                                          \
  } while (0)

static long long r8(long long n) { return (n + 7) / 8 * 8; }

// the header's formulas, restated (tests/test_shoc_coupling_gpu.py, _doubles of tests/test_p3_coupling_gpu.py)
static long long shoc_doubles(long long N, long long Z, long long T) {
  return 10 * r8(N) + r8(T * N) + 22 * r8(Z * N) + r8(2 * Z * N) + r8(T * Z * N) + 11 * r8((Z + 1) * N) + 47 * 8;
}
static long long p3_doubles(long long N, long long Z, long long T) {
  return 37 * r8(Z * N) + 2 * r8(N) + 2 * r8((Z + 1) * N) + r8(3 * N) + 43 * 8 + (T ? r8(T * Z * N) + 8 : 0);
}

// what carve promises, for any sizes: the first slot after one guard, every slot on a multiple of 8, consecutive slots apart by the
// rounded size plus one guard, one guard after the last, and a zero-size array treated as the policy says
static void check_carve(const char *what, const std::vector<long long> &size, cw::ZeroSize policy, long long want_total) {
  const int n = (int)size.size(), guard = cw::GUARD;
  std::vector<long long> offset(n, -7);
  const long long total = cw::carve(size.data(), n, guard, policy, offset.data());
  long long end = 0;   // where the previous slot's rounded array ends
  bool first = true;
  int slots = 0;
  for (int i = 0; i < n; i++) {
    if (size[i] == 0 && policy == cw::ZeroSize::NO_SLOT) {
      CHECK(offset[i] == -1, "%s: array %d has no element and no slot, offset %lld", what, i, offset[i]);
      continue;
    }
    CHECK(offset[i] >= 0 && offset[i] % 8 == 0, "%s: array %d at %lld", what, i, offset[i]);
    if (first) CHECK(offset[i] == guard, "%s: the first array at %lld", what, offset[i]);
    else CHECK(offset[i] == end + guard, "%s: array %d at %lld, the one before ends at %lld", what, i, offset[i], end);
    CHECK(r8(size[i]) - size[i] >= 0 && r8(size[i]) - size[i] < 8, "%s: slack of array %d", what, i);
    end = offset[i] + r8(size[i]);
    first = false;
    slots++;
  }
  CHECK(total == end + guard, "%s: total %lld, the last array ends at %lld", what, total, end);
  CHECK(total % 8 == 0, "%s: total %lld", what, total);
  CHECK(total == want_total, "%s: total %lld, the formula gives %lld (%d slots)", what, total, want_total, slots);
}

// a table: every pointer of the struct once and in the struct's order (the order of the allocation), its sizes under its policy
template <class ARGS, int NA>
static void check_table(const char *what, const cw::Array<ARGS> (&table)[NA], double *ARGS::*first, double *ARGS::*last, long long N, long long Z,
                        long long T, cw::ZeroSize policy, long long want_total) {
  ARGS args = {};
  CHECK(&(args.*table[0].ptr) == &(args.*first) && &(args.*table[NA - 1].ptr) == &(args.*last) && &(args.*last) - &(args.*first) == NA - 1,
        "%s: the table does not span the struct's pointers", what);
  for (int i = 1; i < NA; i++)
    CHECK(&(args.*table[i].ptr) == &(args.*table[i - 1].ptr) + 1, "%s: row %d is not the struct's next pointer", what, i);
  std::vector<long long> size(NA);
  for (int i = 0; i < NA; i++) size[i] = cw::count(table[i].extent, N, Z, T);
  check_carve(what, size, policy, want_total);
  long long offset[NA];
  const long long total = cw::carve_table(table, N, Z, T, policy, offset);
  CHECK(total == want_total, "%s: carve_table gives %lld, the formula %lld", what, total, want_total);
  for (int i = 0; i < NA; i++) {
    const bool none = size[i] == 0 && policy == cw::ZeroSize::NO_SLOT;
    CHECK((offset[i] < 0) == none && cw::may_be_null(table[i], N, Z, T, policy) == none, "%s: row %d, size %lld, offset %lld", what, i, size[i],
          offset[i]);
  }
}

template <class ARGS, int NA> static int row_of(const cw::Array<ARGS> (&table)[NA], double *ARGS::*ptr) {
  for (int i = 0; i < NA; i++)
    if (table[i].ptr == ptr) return i;
  return -1;
}

int main() {
  const int shapes[3][4] = {{3, 5, 1, 7}, {3, 5, 2, 7}, {4, 2, 1, 3}};   // nens, nx, ny, nz: 15, 30 and 8 columns
  char what[96];
  for (const auto &s : shapes) {
    const long long N = (long long)s[0] * s[1] * s[2], Z = s[3];
    for (long long T : {0, 1, 7}) {
      std::snprintf(what, sizeof what, "shoc %dx%dx%dx%d, %lld tracers", s[0], s[1], s[2], s[3], T);
      check_table(what, cw::SHOC_TABLE, &pam_amd_shoc_args_t::host_dx, &pam_amd_shoc_args_t::exner, N, Z, T, cw::SHOC_ZERO_SIZE, shoc_doubles(N, Z, T));
      long long offset[cw::SHOC_NARRAYS];
      cw::carve_table(cw::SHOC_TABLE, N, Z, T, cw::SHOC_ZERO_SIZE, offset);
      const int ws = row_of(cw::SHOC_TABLE, &pam_amd_shoc_args_t::wtracer_sfc), qt = row_of(cw::SHOC_TABLE, &pam_amd_shoc_args_t::qtracers);
      if (T == 0)   // wtracer_sfc and qtracers keep a slot of their own: one guard and nothing else
        CHECK(offset[ws] >= 0 && offset[ws + 1] - offset[ws] == cw::GUARD && offset[qt] >= 0 && offset[qt + 1] - offset[qt] == cw::GUARD, "%s", what);
    }
    for (long long T : {0, 49}) {
      std::snprintf(what, sizeof what, "p3 %dx%dx%dx%d, %lld tendency planes", s[0], s[1], s[2], s[3], T);
      check_table(what, cw::P3_TABLE, &pam_amd_p3_args_t::qc, &pam_amd_p3_args_t::exner, N, Z, T, cw::P3_ZERO_SIZE, p3_doubles(N, Z, T));
      long long offset[cw::P3_NARRAYS];
      cw::carve_table(cw::P3_TABLE, N, Z, T, cw::P3_ZERO_SIZE, offset);
      const int to = row_of(cw::P3_TABLE, &pam_amd_p3_args_t::p3_tend_out);
      CHECK((offset[to] < 0) == (T == 0), "%s: p3_tend_out at %lld", what, offset[to]);
    }
    // the other policy on the same sizes, and bare size lists with empty arrays first, last and side by side
    for (cw::ZeroSize policy : {cw::ZeroSize::KEEP_SLOT, cw::ZeroSize::NO_SLOT}) {
      const bool keep = policy == cw::ZeroSize::KEEP_SLOT;
      std::vector<long long> size(cw::SHOC_NARRAYS);
      for (int i = 0; i < cw::SHOC_NARRAYS; i++) size[i] = cw::count(cw::SHOC_TABLE[i].extent, N, Z, 0);
      check_carve("shoc sizes without tracers, either policy", size, policy, shoc_doubles(N, Z, 0) - (keep ? 0 : 2 * cw::GUARD));
      size.resize(cw::P3_NARRAYS);
      for (int i = 0; i < cw::P3_NARRAYS; i++) size[i] = cw::count(cw::P3_TABLE[i].extent, N, Z, 0);
      check_carve("p3 sizes without tendency planes, either policy", size, policy, p3_doubles(N, Z, 0) + (keep ? cw::GUARD : 0));
      check_carve("empty arrays at both ends", {0, N, 0, 0, Z * N + 1, 0}, policy, (keep ? 7 : 3) * cw::GUARD + r8(N) + r8(Z * N + 1));
      check_carve("nothing but empty arrays", {0, 0}, policy, (keep ? 3 : 1) * cw::GUARD);
    }
  }
  if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
  else std::printf("coupling layout: every check held\n");
  return failures ? 1 : 0;
}
