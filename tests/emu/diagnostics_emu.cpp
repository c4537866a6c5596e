// diagnostics_emu.cpp -- HOST EMULATION of the field diagnostics' device bodies (pam_amd/csrc/diagnostics_device.h, compiled with g++ and
// -ffp-contract=off).  TEST INFRASTRUCTURE ONLY (never shipped, never linked into libpam_amd_awfl.so).  The grids of the four kernels of
// modules_kernels.hip are walked serially with the launch code's own plan of the scratch: every thread runs its share of a chunk, the
// lanes are folded as the header's tree says (`for d = W/2 .. 1: lane[l] += lane[l + d]`, what the shuffles and the LDS hand-off do),
// the extremes by extreme_merge.
#include <algorithm>
#include <vector>

#include "../../pam_amd/csrc/diagnostics_device.h"

using namespace pama::diagnostics;

namespace {

double fold_lanes(double *lane, int W) {
  for (int d = W / 2; d >= 1; d /= 2)
    for (int l = 0; l < d; l++) lane[l] += lane[l + d];
  return lane[0];
}

// one chunk of a vector by the 64 threads of a wavefront; r: the threads' running extremes
template <class T, bool TRACK>
double wave_chunk(const T *p, long long n, long long chunk, int pass, Running<T> *r) {
  double lane[FIELD_W];
  Running<T> unused;
  for (int ln = 0; ln < WAVE; ln++) field_chunk_thread<T, TRACK>(p, n, chunk, ln, pass, lane + FIELD_OWN * ln, TRACK ? r[ln] : unused);
  return fold_lanes(lane, FIELD_W);
}

template <class T>
void field_first(const T *p, long long n, long long nwaves, double *s1, Extreme *ext) {
  const long long nchunks = ceil_div(n, FIELD_CHUNK);
  for (long long gw = 0; gw < nwaves; gw++) {
    Running<T> r[WAVE];
    for (int ln = 0; ln < WAVE; ln++) running_clear(r[ln]);
    int pass = 0;
    for (long long c = gw; c < nchunks; c += nwaves, pass++) s1[c] = wave_chunk<T, true>(p, n, c, pass, r);
    Extreme e;
    extreme_clear(e);
    for (int ln = WAVE - 1; ln >= 0; ln--) {          // any order gives the same
      Extreme t;
      field_finish(r[ln], gw, nwaves, ln, t);
      extreme_merge(e, t);
    }
    ext[gw] = e;
  }
}

void field_second(double *sums, long long cnt, const Extreme *ext, long long next, Result &out) {
  while (cnt > 1) {
    const long long more = ceil_div(cnt, FIELD_CHUNK);
    for (long long c = 0; c < more; c++) sums[cnt + c] = wave_chunk<double, false>(sums, cnt, c, 0, nullptr);
    sums += cnt;
    cnt = more;
  }
  Extreme e;
  extreme_clear(e);
  for (long long w = 0; w < next; w++) extreme_merge(e, ext[w]);
  out = Result{e.vmin, e.vmax, sums[0], e.imin, e.imax, e.nans};
}

// the row chunks chunk0 .. chunk0 + count - 1 of a rows x M array for member m by its four threads: sums[k] of chunk chunk0 + k, and
// (TRACK) the threads' extremes over all of them
template <class T, bool TRACK>
void member_chunks(const T *p, long long rows, long long M, long long chunk0, int count, long long m, double *sums, Extreme *found) {
  double lane[MEMBER_GROUP][MEMBER_W];
  if (TRACK) extreme_clear(*found);
  for (int phase = 0; phase < MEMBER_W; phase++) {
    Running<T> r;
    running_clear(r);
    for (int k = 0; k < count; k++) member_chunk_thread<T, TRACK>(p, rows, M, chunk0 + k, m, phase, k * MEMBER_K, lane[k][phase], r);
    if (TRACK) {
      Extreme t;
      member_finish(r, M, chunk0, m, phase, t);
      extreme_merge(*found, t);
    }
  }
  for (int k = 0; k < count; k++) sums[k] = fold_lanes(lane[k], MEMBER_W);
}

template <class T>
void member_first(const T *p, long long rows, long long M, double *s1, Extreme *ext) {
  const long long n1 = ceil_div(rows, MEMBER_CHUNK);
  for (long long g = 0; g * MEMBER_GROUP < n1; g++)
    for (long long m = 0; m < M; m++) {
      const int count = (int)std::min<long long>(MEMBER_GROUP, n1 - g * MEMBER_GROUP);
      double sums[MEMBER_GROUP];
      member_chunks<T, true>(p, rows, M, g * MEMBER_GROUP, count, m, sums, &ext[g * M + m]);
      for (int k = 0; k < count; k++) s1[(g * MEMBER_GROUP + k) * M + m] = sums[k];
    }
}

void member_second(double *sums, long long n1, long long M, const Extreme *ext, Result *out) {
  long long cnt = n1;
  while (cnt > 1) {
    const long long more = ceil_div(cnt, MEMBER_CHUNK);
    for (long long c = 0; c < more; c++)
      for (long long m = 0; m < M; m++) member_chunks<double, false>(sums, cnt, M, c, 1, m, &sums[(cnt + c) * M + m], nullptr);
    sums += cnt * M;
    cnt = more;
  }
  for (long long m = 0; m < M; m++) {
    Extreme e;
    extreme_clear(e);
    for (long long g = 0; g < ceil_div(n1, MEMBER_GROUP); g++) extreme_merge(e, ext[g * M + m]);
    out[m] = Result{e.vmin, e.vmax, sums[m], e.imin, e.imax, e.nans};
  }
}

}  // namespace

extern "C" {

// The whole call of pam_amd_field_diagnostics on host arrays: `per_launch` fields per launch table (32 in the library), `grid` > 0
// overrides the whole-field launches' workgroups per field.  out: num_fields * max(members, 1) results, NOT_FOUND as -1.
int emu_field_diagnostics(int num_fields, const int *kind, const long long *size, const void *const *data, int members, int per_launch,
                          long long grid, Result *out) {
  const long long M = members < 1 ? 1 : members;
  const int ngroups = (num_fields + per_launch - 1) / per_launch;
  std::vector<FieldPlan> plan(num_fields);
  std::vector<long long> grids(ngroups);
  long long bytes = 0;
  for (int g = 0; g < ngroups; g++) {
    const int f0 = g * per_launch, nf = std::min(per_launch, num_fields - f0);
    long long nmax = 1;
    for (int l = 0; l < nf; l++) nmax = std::max(nmax, size[f0 + l]);
    grids[g] = grid > 0 ? grid : field_grid(nmax, nf);
    for (int l = 0; l < nf; l++) bytes = plan_field(size[f0 + l], members, grids[g] * WAVES, bytes, plan[f0 + l]);
  }
  std::vector<double> storage(bytes / 8 + 2);            // 8-byte aligned is all the host needs
  char *base = (char *)storage.data();
  for (int f = 0; f < num_fields; f++) {
    double *sums = (double *)(base + plan[f].sums_off);
    Extreme *ext = (Extreme *)(base + plan[f].ext_off);
    const long long nwaves = grids[f / per_launch] * WAVES;
    if (members < 1) {
      if (kind[f] == KIND_DOUBLE) field_first((const double *)data[f], size[f], nwaves, sums, ext);
      else field_first((const float *)data[f], size[f], nwaves, sums, ext);
      field_second(sums, plan[f].n1, ext, nwaves, out[f]);
    } else {
      if (kind[f] == KIND_DOUBLE) member_first((const double *)data[f], size[f] / M, M, sums, ext);
      else member_first((const float *)data[f], size[f] / M, M, sums, ext);
      member_second(sums, plan[f].n1, M, ext, out + (long long)f * M);
    }
  }
  for (long long i = 0; i < num_fields * M; i++) {
    if (out[i].imin == NOT_FOUND) out[i].imin = -1;
    if (out[i].imax == NOT_FOUND) out[i].imax = -1;
  }
  return 0;
}

}
