// validate_device.h -- the state check of DataManager::validate / validate_all (pam_core/DataManager.h:408-509) as PAMA_D functions:
// the per-element classification, one thread's walk over its share of a field, and the fold of the threads' findings.  The HIP kernel
// in modules_kernels.hip calls them (it keeps the wavefront shuffle, the LDS hand-off and the atomics), and tests/emu/validate_emu.cpp
// compiles the same bodies with g++ and walks the grid serially.
//   validate_single_nan   DataManager.h:471-479   std::isnan(x)                       floating kinds
//   validate_single_inf   DataManager.h:484-492   std::isinf(x), either sign           floating kinds
//   validate_single_pos   DataManager.h:497-509   x < 0. where the entry is positive   every kind
// so -inf is inf AND negative; -0.0 and a NaN with the sign bit set are not negative.  Everything is an integer: per field and class
// the number of offenders and the lowest flat index of one, exact and the same from run to run.  Indices are 64-bit throughout (the
// reference's `int i` wraps past 2^31 elements).
#pragma once
#include <string.h>

#if !defined(PAMA_D)
#if defined(__HIPCC__)
#define PAMA_D __device__ __forceinline__
#else
#define PAMA_D inline
#endif
#endif

namespace pama {
namespace validate {

constexpr int KIND_DOUBLE = 0, KIND_FLOAT = 1, KIND_INT = 2, KIND_LONGLONG = 3;
constexpr int NAN_CLASS = 0, INF_CLASS = 1, NEG_CLASS = 2, NUM_CLASSES = 3;
constexpr int THREADS = 256;   // threads of a workgroup
constexpr int UNROLL = 4;      // 16-byte loads a thread has in flight per pass
constexpr long long NOT_FOUND = 0x7fffffffffffffffLL;

// what one thread, one wavefront, one workgroup has found so far
struct Tally {
  long long count[NUM_CLASSES];
  long long first[NUM_CLASSES];   // lowest flat index, NOT_FOUND where count is 0
};

PAMA_D void tally_clear(Tally &t) {
  for (int c = 0; c < NUM_CLASSES; c++) { t.count[c] = 0; t.first[c] = NOT_FOUND; }
}

// the fold: counts add, first indices take the minimum (associative and commutative, so any order gives the same integers)
PAMA_D void tally_merge(Tally &a, const Tally &b) {
  for (int c = 0; c < NUM_CLASSES; c++) {
    a.count[c] += b.count[c];
    a.first[c] = b.first[c] < a.first[c] ? b.first[c] : a.first[c];
  }
}

PAMA_D bool tally_any(const Tally &t) { return (t.count[0] | t.count[1] | t.count[2]) != 0; }

// bit c set: the element is an offender of class c
PAMA_D unsigned classify(double x, bool positive) {
  unsigned long long b;
  memcpy(&b, &x, 8);
  const unsigned long long a = b & 0x7fffffffffffffffULL;
  return (a > 0x7ff0000000000000ULL ? 1u : 0u) | (a == 0x7ff0000000000000ULL ? 2u : 0u) | ((positive && x < 0.0) ? 4u : 0u);
}
PAMA_D unsigned classify(float x, bool positive) {
  unsigned b;
  memcpy(&b, &x, 4);
  const unsigned a = b & 0x7fffffffu;
  return (a > 0x7f800000u ? 1u : 0u) | (a == 0x7f800000u ? 2u : 0u) | ((positive && x < 0.0f) ? 4u : 0u);
}
PAMA_D unsigned classify(int x, bool positive) { return (positive && x < 0) ? 4u : 0u; }
PAMA_D unsigned classify(long long x, bool positive) { return (positive && x < 0) ? 4u : 0u; }

PAMA_D void tally_add(Tally &t, unsigned bits, long long index) {
  for (int c = 0; c < NUM_CLASSES; c++)
    if (bits >> c & 1u) {
      t.count[c]++;
      t.first[c] = index < t.first[c] ? index : t.first[c];
    }
}

// 16 bytes of a field, loaded at once
template <class T>
struct alignas(16) Vec16 { T v[16 / sizeof(T)]; };

// How a field of n elements at address `addr` (aligned to its element) is cut: `head` elements up to the first 16-byte boundary, `nvec`
// whole 16-byte vectors, `tail` elements after them.  A view t[1:] of an f32 tensor has head = 3.
struct Cut { long long head, nvec, tail; };
template <class T>
PAMA_D Cut cut_field(unsigned long long addr, long long n) {
  constexpr long long PER = 16 / sizeof(T);
  Cut c;
  c.head = (long long)(((16 - (addr & 15)) & 15) / sizeof(T));
  if (c.head > n) c.head = n;
  c.nvec = (n - c.head) / PER;
  c.tail = n - c.head - c.nvec * PER;
  return c;
}

// one 16-byte vector whose first element has flat index i0: classified; the tally is touched only where something was found
template <class T>
PAMA_D void scan_vector(const Vec16<T> &x, bool positive, long long i0, Tally &t) {
  constexpr int PER = (int)(16 / sizeof(T));
  unsigned any = 0;
  for (int e = 0; e < PER; e++) any |= classify(x.v[e], positive);
  if (any)
    for (int e = 0; e < PER; e++) tally_add(t, classify(x.v[e], positive), i0 + e);
}

// The walk of thread `tid` of workgroup `block` (of `nblocks`) over a field: the workgroups stride over the whole vectors in passes of
// THREADS x UNROLL vectors, lane after lane on consecutive vectors; the head and tail elements (at most 2 x (16/sizeof(T) - 1)) go to
// the first threads of workgroup 0, one element each.  Reads only.  A whole pass (the same for every thread of the workgroup) issues
// its UNROLL loads before it looks at any of them; the last, partial pass of a field checks every vector against the end.  A vector
// without an offender costs its classification and one branch.
template <class T>
PAMA_D void thread_scan(const T *p, long long n, bool positive, long long block, long long nblocks, int tid, Tally &t) {
  constexpr int PER = (int)(16 / sizeof(T));
  constexpr long long PASS = (long long)THREADS * UNROLL;
  const Cut c = cut_field<T>((unsigned long long)p, n);
  if (block == 0 && tid < c.head + c.tail) {
    const long long i = tid < c.head ? (long long)tid : c.head + c.nvec * PER + ((long long)tid - c.head);
    const unsigned bits = classify(p[i], positive);
    if (bits) tally_add(t, bits, i);
  }
  const Vec16<T> *body = reinterpret_cast<const Vec16<T> *>(p + c.head);
  for (long long b0 = block * PASS; b0 < c.nvec; b0 += nblocks * PASS) {
    const long long v0 = b0 + tid;
    if (b0 + PASS <= c.nvec) {
      Vec16<T> x[UNROLL];
#if defined(__clang__)
#pragma unroll
#endif
      for (int j = 0; j < UNROLL; j++) x[j] = body[v0 + (long long)(j * THREADS)];
#if defined(__clang__)
#pragma unroll
#endif
      for (int j = 0; j < UNROLL; j++) scan_vector(x[j], positive, c.head + (v0 + (long long)(j * THREADS)) * PER, t);
    } else {
      for (int j = 0; j < UNROLL; j++) {
        const long long v = v0 + (long long)(j * THREADS);
        if (v < c.nvec) scan_vector(body[v], positive, c.head + v * PER, t);
      }
    }
  }
}

// thread_scan by element kind; an unknown kind finds nothing (the entry points refuse it before a launch)
PAMA_D void thread_scan_kind(int kind, const void *p, long long n, bool positive, long long block, long long nblocks, int tid, Tally &t) {
  switch (kind) {
    case KIND_DOUBLE: thread_scan((const double *)p, n, positive, block, nblocks, tid, t); break;
    case KIND_FLOAT: thread_scan((const float *)p, n, positive, block, nblocks, tid, t); break;
    case KIND_INT: thread_scan((const int *)p, n, positive, block, nblocks, tid, t); break;
    case KIND_LONGLONG: thread_scan((const long long *)p, n, positive, block, nblocks, tid, t); break;
    default: break;
  }
}

// (constexpr: callable from the host's launch code and from the device alike)
constexpr int kind_bytes(int kind) { return (kind == KIND_DOUBLE || kind == KIND_LONGLONG) ? 8 : 4; }

// workgroups a field of n elements can keep busy (one pass of THREADS x UNROLL vectors each), at least 1
constexpr long long blocks_needed(int kind, long long n) {
  const long long per = (long long)(THREADS * UNROLL) * (16 / kind_bytes(kind));
  return (n + per - 1) / per < 1 ? 1 : (n + per - 1) / per;
}

}  // namespace validate
}  // namespace pama
