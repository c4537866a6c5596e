// diagnostics_device.h -- the field diagnostics (pam_amd_field_diagnostics: least and greatest element with their flat indices, the
// number of NaNs and a REPRODUCIBLE sum, per field or per ensemble member) as PAMA_D functions: the per-element update, a thread's share
// of one chunk, and the folds.  The HIP kernels in modules_kernels.hip call them (they keep the wavefront shuffles, the LDS hand-off and
// the launch code), and tests/emu/diagnostics_emu.cpp compiles the same bodies with g++ and walks the grids serially.  The counterpart
// of the reference's DEBUG_PRINT_SUM / AVG / MIN / MAX (pam_core/pam_const.h:308-333; yakl::intrinsics::sum / minval / maxval).
//
// THE SUM TREE is a contract: it depends on the element values and their flat index alone, not on the grid, the split of a field list,
// the base address or the device.  fold(v; W, K): v is cut into chunks of W*K consecutive entries; entry e of a chunk belongs to virtual
// lane e % W at step e / W; a lane adds its K entries in ascending step order; the lanes are folded by
// `for d = W/2 .. 1: lane[l] += lane[l + d]` (l < d); the chunk results form the next v, until one value is left (a vector of one chunk
// takes one level).  A missing entry counts as -0.0, the identity of IEEE addition, so it may as well be skipped.
//   whole field   W = 256, K = 8  over the flat index.  A wavefront owns a chunk: thread t holds the lanes 4t .. 4t+3 (consecutive
//                 elements, so its loads are 16 bytes wide; a double's 32 bytes take two), the steps d = 128 .. 4 of the lane fold
//                 are `thread t += thread t + d/4`, six wavefront shuffles, and d = 2, 1 happen inside thread 0.
//   per member    W = 4, K = 64   over the row index r of x[r*M + m], for each m.  A thread is a (member, row phase) pair: wavefront
//                 p of a workgroup holds lane p of 64 consecutive members, and the four lanes are folded through LDS.
//                 A workgroup takes MEMBER_GROUP consecutive row chunks, so that it leaves a quarter as many extremes.
// The first launch writes the level-1 chunk results; they are a vector (or a rows x M array) like the field itself, so the second launch
// folds the remaining levels with the same bodies.  Floats are converted to double exactly before they are added.
//
// MIN AND MAX.  NaNs take no part (they are counted); infinities do.  Among elements that compare equal the lowest flat index wins, and
// the value is that element's own bits.  A thread visits its elements in ascending index order and replaces its extreme on a strict
// comparison; its "nothing yet" is a NaN extreme, which `!(x >= vmin)` replaces by the first element that is no NaN (a +inf included).
// Threads, wavefronts and workgroups fold by the lexicographic comparison of (value, index), which is associative and commutative.
#pragma once
#include <string.h>

#if !defined(PAMA_D)
#if defined(__HIPCC__)
#define PAMA_D __device__ __forceinline__
#else
#define PAMA_D inline
#endif
#endif

#if defined(__clang__)
#define PAMA_DIAG_UNROLL _Pragma("unroll")
#else
#define PAMA_DIAG_UNROLL
#endif

namespace pama {
namespace diagnostics {

constexpr int KIND_DOUBLE = 0, KIND_FLOAT = 1;
constexpr int THREADS = 256, WAVE = 64, WAVES = THREADS / WAVE;
constexpr int FIELD_W = 256, FIELD_K = 8, FIELD_CHUNK = FIELD_W * FIELD_K;       // the whole-field tree
constexpr int FIELD_OWN = FIELD_W / WAVE;                                         // lanes of the tree a thread holds: 4
constexpr int MEMBER_W = 4, MEMBER_K = 64, MEMBER_CHUNK = MEMBER_W * MEMBER_K;   // the per-member tree
constexpr int MEMBER_TILE = WAVE;                                                 // members of a workgroup
constexpr int MEMBER_GROUP = 4;   // consecutive row chunks a workgroup of the first launch takes: one extreme per (group, member)
constexpr long long NOT_FOUND = 0x7fffffffffffffffLL;
static_assert(FIELD_OWN == 4 && MEMBER_W == WAVES && MEMBER_GROUP == WAVES, "the kernels' thread layout");

// what a wavefront, a workgroup or a field has found: float values converted exactly; NOT_FOUND where every element was a NaN
struct Extreme {
  double vmin, vmax;
  long long imin, imax, nans;
};
// what comes back per (field, member)
struct Result {
  double vmin, vmax, vsum;
  long long imin, imax, nans;
};

PAMA_D void extreme_clear(Extreme &e) {
  e.vmin = __builtin_inf();
  e.vmax = -__builtin_inf();
  e.imin = e.imax = NOT_FOUND;
  e.nans = 0;
}

// field by field (a struct assignment to LDS or global memory keeps the compiler from holding the struct in registers)
PAMA_D void extreme_copy(Extreme &to, const Extreme &from) {
  to.vmin = from.vmin;
  to.vmax = from.vmax;
  to.imin = from.imin;
  to.imax = from.imax;
  to.nans = from.nans;
}

// lexicographic (value, index): the lower index wins among equal values, for the maximum too.  (The other side comes as values, read
// before any comparison: selecting between two structs by reference keeps both in memory.)
PAMA_D void extreme_merge_values(Extreme &a, double vmin, double vmax, long long imin, long long imax, long long nans) {
  const bool lo = vmin < a.vmin || (vmin == a.vmin && imin < a.imin);
  const bool hi = vmax > a.vmax || (vmax == a.vmax && imax < a.imax);
  a.vmin = lo ? vmin : a.vmin;
  a.imin = lo ? imin : a.imin;
  a.vmax = hi ? vmax : a.vmax;
  a.imax = hi ? imax : a.imax;
  a.nans += nans;
}
PAMA_D void extreme_merge(Extreme &a, const Extreme &b) { extreme_merge_values(a, b.vmin, b.vmax, b.imin, b.imax, b.nans); }

// one thread's extremes so far, in the element's own type; q: the ordinal of the element in the thread's walk, -1: nothing yet
template <class T>
struct Running {
  T vmin, vmax;
  int qmin, qmax;
  long long nans;
};

template <class T>
PAMA_D void running_clear(Running<T> &r) {
  r.vmin = r.vmax = (T)__builtin_nan("");
  r.qmin = r.qmax = -1;
  r.nans = 0;
}

// the per-element update; `q` ascends along the thread's walk, `nans` is the caller's count for the chunk
template <class T>
PAMA_D void running_update(Running<T> &r, T x, int q, int &nans) {
  const bool ok = x == x;
  const bool lo = ok & !(x >= r.vmin);
  const bool hi = ok & !(x <= r.vmax);
  nans += ok ? 0 : 1;
  r.vmin = lo ? x : r.vmin;
  r.qmin = lo ? q : r.qmin;
  r.vmax = hi ? x : r.vmax;
  r.qmax = hi ? q : r.qmax;
}

// the last two steps of a four-lane fold: d = 2 (lane 0 += lane 2, lane 1 += lane 3), then d = 1
PAMA_D double fold4(double a0, double a1, double a2, double a3) { return (a0 + a2) + (a1 + a3); }

constexpr long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

// entries of all level buffers of a vector whose level 1 has n1 chunk results: n1 + n2 + ... + 1
constexpr long long level_entries(long long n1, long long chunk) {
  long long total = n1;
  while (n1 > 1) {
    n1 = ceil_div(n1, chunk);
    total += n1;
  }
  return total;
}

// ------------------------------------------------------------------------------------------------------------------------------
// whole field

// Thread `ln` (0 .. 63) of the wavefront that owns chunk `chunk` of the vector p[0 .. n): acc[j] is the sum of lane 4*ln + j over
// its K steps.  A whole chunk issues all its loads before it looks at any of them (FIELD_OWN consecutive elements each: the address
// is aligned to the element only, which global loads of 16 bytes allow); the last, partial chunk checks every element against the end.
// TRACK: the elements also update `r`, with the ordinals pass*32 .. pass*32 + 31 in ascending index order.
template <class T, bool TRACK>
PAMA_D void field_chunk_thread(const T *p, long long n, long long chunk, int ln, int pass, double acc[FIELD_OWN], Running<T> &r) {
  const long long base = chunk * FIELD_CHUNK + (long long)(FIELD_OWN * ln);
  int nans = 0;
  for (int j = 0; j < FIELD_OWN; j++) acc[j] = -0.0;
  if ((chunk + 1) * FIELD_CHUNK <= n) {
    T x[FIELD_K][FIELD_OWN];
    PAMA_DIAG_UNROLL
    for (int s = 0; s < FIELD_K; s++) memcpy(x[s], p + base + (long long)(s * FIELD_W), sizeof(x[s]));
    PAMA_DIAG_UNROLL
    for (int s = 0; s < FIELD_K; s++) {
      PAMA_DIAG_UNROLL
      for (int j = 0; j < FIELD_OWN; j++) {
        acc[j] += (double)x[s][j];
        if (TRACK) running_update(r, x[s][j], (pass * FIELD_K + s) * FIELD_OWN + j, nans);
      }
    }
  } else {
    // the same with every element checked; a missing one is loaded as -0.0 and added (the identity), and updates nothing
    T x[FIELD_K][FIELD_OWN];
    PAMA_DIAG_UNROLL
    for (int s = 0; s < FIELD_K; s++) {
      PAMA_DIAG_UNROLL
      for (int j = 0; j < FIELD_OWN; j++) {
        const long long i = base + (long long)(s * FIELD_W + j);
        x[s][j] = i < n ? p[i] : (T)-0.0;
      }
    }
    PAMA_DIAG_UNROLL
    for (int s = 0; s < FIELD_K; s++) {
      PAMA_DIAG_UNROLL
      for (int j = 0; j < FIELD_OWN; j++) {
        acc[j] += (double)x[s][j];
        if (TRACK && base + (long long)(s * FIELD_W + j) < n) running_update(r, x[s][j], (pass * FIELD_K + s) * FIELD_OWN + j, nans);
      }
    }
  }
  if (TRACK) r.nans += nans;
}

// the flat index of ordinal q of thread `ln` of wavefront `gw` of `nwaves`, which took the chunks gw, gw + nwaves, ...
PAMA_D long long field_index(int q, long long gw, long long nwaves, int ln) {
  const int per = FIELD_K * FIELD_OWN;
  const long long chunk = gw + (long long)(q / per) * nwaves;
  return chunk * FIELD_CHUNK + (long long)((q % per) / FIELD_OWN * FIELD_W + FIELD_OWN * ln + q % FIELD_OWN);
}

template <class T>
PAMA_D void field_finish(const Running<T> &r, long long gw, long long nwaves, int ln, Extreme &e) {
  extreme_clear(e);
  if (r.qmin >= 0) {
    e.vmin = (double)r.vmin;
    e.imin = field_index(r.qmin, gw, nwaves, ln);
    e.vmax = (double)r.vmax;
    e.imax = field_index(r.qmax, gw, nwaves, ln);
  }
  e.nans = r.nans;
}

// workgroups per field of a launch of `nf` fields whose largest has `nmax` elements: ~2048 workgroups in all (eight per CU), never
// more than the largest field has chunks for, never so few that a thread's ordinals overflow
constexpr long long field_grid(long long nmax, int nf) {
  const long long need = ceil_div(ceil_div(nmax, FIELD_CHUNK), WAVES);
  long long g = 2048 / nf < 1 ? 1 : 2048 / nf;
  g = g < need ? g : need;
  const long long least = ceil_div(ceil_div(nmax, FIELD_CHUNK), (long long)WAVES << 25);
  g = g < least ? least : g;
  return g < 1 ? 1 : g;
}

// ------------------------------------------------------------------------------------------------------------------------------
// per member: p is rows x M, the member the fastest axis

// Thread (member m, row phase `phase`) of the workgroup that owns row chunk `chunk`: acc is the sum of lane `phase`, the rows
// chunk*256 + 4*s + phase for s = 0 .. 63 in ascending order; TRACK: the elements update `r` with the ordinal q0 + s.  A partial chunk keeps
// its loads in flight like a whole one: the levels the second launch folds are mostly partial chunks.
template <class T, bool TRACK>
PAMA_D void member_chunk_thread(const T *p, long long rows, long long M, long long chunk, long long m, int phase, int q0, double &acc,
                                Running<T> &r) {
  constexpr int UNROLL = 16;
  const long long r0 = chunk * MEMBER_CHUNK + phase;
  int nans = 0;
  acc = -0.0;
  if ((chunk + 1) * MEMBER_CHUNK <= rows) {
    for (int s0 = 0; s0 < MEMBER_K; s0 += UNROLL) {
      T x[UNROLL];
      PAMA_DIAG_UNROLL
      for (int u = 0; u < UNROLL; u++) x[u] = p[(r0 + (long long)(MEMBER_W * (s0 + u))) * M + m];
      PAMA_DIAG_UNROLL
      for (int u = 0; u < UNROLL; u++) {
        acc += (double)x[u];
        if (TRACK) running_update(r, x[u], q0 + s0 + u, nans);
      }
    }
  } else {
    // the same with every row checked, UNROLL loads in flight all the same: a missing entry is loaded as -0.0 and added (the
    // identity), and updates nothing
    for (int s0 = 0; s0 < MEMBER_K; s0 += UNROLL) {
      T x[UNROLL];
      PAMA_DIAG_UNROLL
      for (int u = 0; u < UNROLL; u++) {
        const long long row = r0 + (long long)(MEMBER_W * (s0 + u));
        x[u] = row < rows ? p[row * M + m] : (T)-0.0;
      }
      PAMA_DIAG_UNROLL
      for (int u = 0; u < UNROLL; u++) {
        acc += (double)x[u];
        if (TRACK && r0 + (long long)(MEMBER_W * (s0 + u)) < rows) running_update(r, x[u], q0 + s0 + u, nans);
      }
    }
  }
  if (TRACK) r.nans += nans;
}

// the extremes of a thread that walked the chunks chunk, chunk + 1, ... with q0 = 0, 64, ...: ordinal q is the row chunk*256 + 4*q + phase
template <class T>
PAMA_D void member_finish(const Running<T> &r, long long M, long long chunk, long long m, int phase, Extreme &e) {
  extreme_clear(e);
  if (r.qmin >= 0) {
    e.vmin = (double)r.vmin;
    e.imin = (chunk * MEMBER_CHUNK + (long long)(MEMBER_W * r.qmin + phase)) * M + m;
    e.vmax = (double)r.vmax;
    e.imax = (chunk * MEMBER_CHUNK + (long long)(MEMBER_W * r.qmax + phase)) * M + m;
  }
  e.nans = r.nans;
}

// ------------------------------------------------------------------------------------------------------------------------------
// the scratch of one call: per field its level buffers (doubles) and the extremes the first launch leaves (one per wavefront, or one
// per (group of MEMBER_GROUP row chunks, member)), then one Result per (field, member).  Offsets in bytes, every region 16-byte aligned.
struct FieldPlan {
  long long n1;         // chunk results of level 1 (per member)
  long long sums_off;   // level buffers: level_entries(n1) x max(M, 1) doubles
  long long ext_off;    // extremes
};

constexpr long long align16(long long b) { return (b + 15) / 16 * 16; }

// the plan of field `size` at byte `at`; members = 0: whole field, `ext_count` wavefronts leave an extreme.  Returns the first byte
// after the field's regions.
inline long long plan_field(long long size, int members, long long ext_count, long long at, FieldPlan &pl) {
  const long long M = members < 1 ? 1 : members;
  const long long chunk = members < 1 ? FIELD_CHUNK : MEMBER_CHUNK;
  pl.n1 = ceil_div(size / M, chunk);
  pl.sums_off = at;
  at = align16(at + level_entries(pl.n1, chunk) * M * (long long)sizeof(double));
  pl.ext_off = at;
  return align16(at + (members < 1 ? ext_count : ceil_div(pl.n1, MEMBER_GROUP) * M) * (long long)sizeof(Extreme));
}

}  // namespace diagnostics
}  // namespace pama
