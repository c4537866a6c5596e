// Serial stand-in for the YAKL array / kernel-launch API.   TEST INFRASTRUCTURE ONLY.
//
// Written for this project from the list of YAKL names the reference headers use.  It lets the
// reference's own headers compile unmodified with g++ and run on one CPU core at IEEE fp64, so that oracle/awfl_oracle.c,
// the HIP kernels and the Python restatements can be compared with the reference's source text (oracle/ref_harness.cpp).
//
// Semantics:
//   * Array<T,N,mem,style>: styleC is row-major (last index fastest).  styleFortran is declared for the typedefs only.
//     Owning arrays share one allocation by reference count; copies are shallow, as in YAKL.
//   * c::parallel_for: nested serial loops, first bound slowest.  atomicAdd is a plain add, so every reduction runs in
//     loop order.
//   * New allocations (owning Array constructors, alloc_device) are filled with NaN by default, so a read of memory the
//     reference never wrote shows up in its outputs.  set_alloc_fill(ALLOC_FILL_ZERO) fills them with zeros instead.
//   * Replay hook: a parallel_for whose label ends in the path component set by set_replay_label() runs its body twice
//     and counts the replays.  This makes the vertical boundary kernel's ghost read-after-write
//     order-independent, as the oracle and the HIP kernels implement it.
//
// NOT pinned by this stand-in (they stay assumptions of the project): intrinsics::matinv_ge (Gauss-Jordan without pivoting,
// deviation D3), the summation order of a device atomicAdd, and minval/maxval/sum beyond serial element order.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#define YAKL_INLINE inline
#define YAKL_LAMBDA [=]
#define YAKL_DEVICE_LAMBDA [=]
#define YAKL_SCOPE(a, b) auto &a = b
#define YAKL_STANDIN_STR2(x) #x
#define YAKL_STANDIN_STR(x) YAKL_STANDIN_STR2(x)
#define YAKL_AUTO_LABEL() (__FILE__ ":" YAKL_STANDIN_STR(__LINE__))

namespace yakl {

typedef unsigned int index_t;
int constexpr memDevice = 1;
int constexpr memHost = 2;
int constexpr styleC = 1;
int constexpr styleFortran = 2;
int constexpr COLON = -1;

int constexpr ALLOC_FILL_NAN = 0;
int constexpr ALLOC_FILL_ZERO = 1;

// Switches of the stand-in, set by the harness.  Defined in exactly one translation unit (YAKL_STANDIN_DEFINE_GLOBALS).
struct StandinState {
  int alloc_fill = ALLOC_FILL_NAN;
  std::string replay_label;   // empty: no replay
  long replay_count = 0;
};
StandinState &standin_state();
#ifdef YAKL_STANDIN_DEFINE_GLOBALS
StandinState &standin_state() {
  static StandinState s;
  return s;
}
#endif

inline void set_alloc_fill(int mode) { standin_state().alloc_fill = mode; }
inline void set_replay_label(char const *label) { standin_state().replay_label = label ? label : ""; }
inline long replay_count() { return standin_state().replay_count; }
inline void reset_replay_count() { standin_state().replay_count = 0; }

inline void fill_new_allocation(void *ptr, size_t bytes) {
  // 0xFF bytes: a quiet NaN for every double and float, -1 for integers.
  std::memset(ptr, standin_state().alloc_fill == ALLOC_FILL_ZERO ? 0 : 0xFF, bytes);
}

[[noreturn]] inline void yakl_throw(char const *msg) { throw std::runtime_error(msg); }

inline void *alloc_device(size_t bytes, char const * = nullptr) {
  void *p = std::malloc(bytes > 0 ? bytes : 1);
  if (!p) yakl_throw("yakl stand-in: allocation failed");
  fill_new_allocation(p, bytes);
  return p;
}
inline void free_device(void *ptr, char const * = nullptr) { std::free(ptr); }
inline void fence() {}
inline void timer_start(char const *) {}
inline void timer_stop(char const *) {}

template <class T> YAKL_INLINE constexpr T min(T a, T b) { return a < b ? a : b; }
template <class T> YAKL_INLINE constexpr T max(T a, T b) { return a > b ? a : b; }

// ---------------------------------------------------------------------------------------------------------------------
// SArray: fixed-size, row-major, value semantics.  operator() returns a mutable reference from a const object, as in YAKL.
template <class T, int rank, unsigned D0, unsigned D1 = 1, unsigned D2 = 1, unsigned D3 = 1>
class SArray {
 public:
  static unsigned constexpr totElems_ = D0 * D1 * D2 * D3;
  mutable T myData[totElems_];

  SArray() = default;
  SArray(T v) { *this = v; }
  SArray &operator=(T v) {
    for (unsigned i = 0; i < totElems_; i++) myData[i] = v;
    return *this;
  }
  YAKL_INLINE T &operator()(index_t i0) const { return myData[i0]; }
  YAKL_INLINE T &operator()(index_t i0, index_t i1) const { return myData[i0 * D1 + i1]; }
  YAKL_INLINE T &operator()(index_t i0, index_t i1, index_t i2) const { return myData[(i0 * D1 + i1) * D2 + i2]; }
  YAKL_INLINE T &operator()(index_t i0, index_t i1, index_t i2, index_t i3) const {
    return myData[((i0 * D1 + i1) * D2 + i2) * D3 + i3];
  }
  static constexpr unsigned size() { return totElems_; }
  static constexpr unsigned totElems() { return totElems_; }
  T *data() const { return myData; }
  friend std::ostream &operator<<(std::ostream &os, SArray const &a) {
    for (unsigned i = 0; i < totElems_; i++) os << a.myData[i] << (i + 1 < totElems_ ? " " : "\n");
    return os;
  }
};

// ---------------------------------------------------------------------------------------------------------------------
template <class T, int N, int MEM = memDevice, int STYLE = styleC>
class Array {
  static_assert(STYLE == styleC, "yakl stand-in: only styleC arrays can be instantiated");

 public:
  typedef typename std::remove_cv<T>::type type;
  T *myData = nullptr;
  int dimension[N > 0 ? N : 1] = {};
  std::shared_ptr<type> owner;
  char const *myname = "";

  Array() = default;

  // owning: (label, d0, ..., dN-1)
  template <class... I, typename std::enable_if<sizeof...(I) == N && (std::is_integral<I>::value && ...), int>::type = 0>
  Array(char const *label, I... dims) : myname(label) {
    int d[N] = {int(dims)...};
    for (int i = 0; i < N; i++) dimension[i] = d[i];
    allocate();
  }
  Array(char const *label, std::vector<int> const &dims) : myname(label) {
    set_dims(dims);
    allocate();
  }
  // non-owning: (label, pointer, d0, ..., dN-1) and (label, pointer, dims)
  template <class... I, typename std::enable_if<sizeof...(I) == N && (std::is_integral<I>::value && ...), int>::type = 0>
  Array(char const *label, T *data, I... dims) : myData(data), myname(label) {
    int d[N] = {int(dims)...};
    for (int i = 0; i < N; i++) dimension[i] = d[i];
  }
  Array(char const *label, T *data, std::vector<int> const &dims) : myData(data), myname(label) { set_dims(dims); }

  // non-const -> const element type
  template <class U, typename std::enable_if<std::is_same<typename std::add_const<U>::type, T>::value &&
                                                 !std::is_same<U, T>::value, int>::type = 0>
  Array(Array<U, N, MEM, STYLE> const &rhs) : myData(rhs.myData), owner(rhs.owner), myname(rhs.myname) {
    for (int i = 0; i < N; i++) dimension[i] = rhs.dimension[i];
  }

  Array(Array const &) = default;
  Array(Array &&) = default;
  Array &operator=(Array const &) = default;
  Array &operator=(Array &&) = default;

  // scalar fill
  Array const &operator=(type v) const {
    for (size_t i = 0; i < totElems(); i++) myData[i] = v;
    return *this;
  }

  // Row-major indexing.  Any index count compiles, so that decltype over 6-8 indices in MultipleFields.h is well-formed
  // for arrays of lower rank; calling with a count other than N is a compile error.
  template <class... I>
  YAKL_INLINE T &operator()(I... ind) const {
    static_assert(sizeof...(I) == N, "yakl stand-in: wrong number of indices");
    size_t idx[N] = {size_t(ind)...};
    size_t off = 0;
    for (int i = 0; i < N; i++) off = off * size_t(dimension[i]) + idx[i];
    return myData[off];
  }

  size_t totElems() const {
    size_t n = 1;
    for (int i = 0; i < N; i++) n *= size_t(dimension[i]);
    return n;
  }
  size_t size() const { return totElems(); }
  size_t get_elem_count() const { return totElems(); }
  int extent(int i) const { return dimension[i]; }
  int get_rank() const { return N; }
  T *data() const { return myData; }
  T *get_data() const { return myData; }
  bool initialized() const { return myData != nullptr; }
  char const *label() const { return myname; }

  template <class... I>
  Array<T, sizeof...(I), MEM, STYLE> reshape(I... dims) const {
    Array<T, sizeof...(I), MEM, STYLE> r(myname, myData, dims...);
    if (r.totElems() != totElems()) yakl_throw("yakl stand-in: reshape changes the element count");
    r.owner = owner;
    return r;
  }

  Array<type, N, memHost, STYLE> createHostCopy() const { return deep_copy_into<memHost>(); }
  Array<type, N, memDevice, STYLE> createDeviceCopy() const { return deep_copy_into<memDevice>(); }

  template <class U, int M2, int S2>
  void deep_copy_to(Array<U, N, M2, S2> const &dst) const {
    if (dst.totElems() != totElems()) yakl_throw("yakl stand-in: deep_copy_to between arrays of different sizes");
    std::memcpy((void *)dst.myData, (void const *)myData, totElems() * sizeof(type));
  }

  friend std::ostream &operator<<(std::ostream &os, Array const &a) {
    os << "Array " << a.myname << ":";
    for (size_t i = 0; i < a.totElems(); i++) os << " " << a.myData[i];
    return os << "\n";
  }

 private:
  void set_dims(std::vector<int> const &dims) {
    if (int(dims.size()) != N) yakl_throw("yakl stand-in: dimension count does not match the array rank");
    for (int i = 0; i < N; i++) dimension[i] = dims[i];
  }
  void allocate() {
    size_t bytes = totElems() * sizeof(type);
    type *p = static_cast<type *>(std::malloc(bytes > 0 ? bytes : 1));
    if (!p) yakl_throw("yakl stand-in: allocation failed");
    fill_new_allocation(p, bytes);
    owner = std::shared_ptr<type>(p, [](type *q) { std::free(q); });
    myData = p;
  }
  template <int M2>
  Array<type, N, M2, STYLE> deep_copy_into() const {
    Array<type, N, M2, STYLE> r;
    r.myname = myname;
    for (int i = 0; i < N; i++) r.dimension[i] = dimension[i];
    size_t bytes = totElems() * sizeof(type);
    type *p = static_cast<type *>(std::malloc(bytes > 0 ? bytes : 1));
    if (!p) yakl_throw("yakl stand-in: allocation failed");
    std::memcpy(p, (void const *)myData, bytes);
    r.owner = std::shared_ptr<type>(p, [](type *q) { std::free(q); });
    r.myData = p;
    return r;
  }
};

inline void memset(void *, int) {}
template <class T, int N, int M, int S, class V>
void memset(Array<T, N, M, S> const &a, V v) {
  a = v;
}

// Scalar written by a kernel and read back on the host.  Kernels capture it by value, so every copy refers to ONE value.
template <class T>
class ScalarLiveOut {
 public:
  std::shared_ptr<T> val;
  ScalarLiveOut() : val(std::make_shared<T>()) {}
  explicit ScalarLiveOut(T v) : val(std::make_shared<T>(v)) {}
  ScalarLiveOut const &operator=(T v) const {
    *val = v;
    return *this;
  }
  T hostRead() const { return *val; }
  void hostWrite(T v) { *val = v; }
  operator T() const { return *val; }
};

template <class T>
YAKL_INLINE T atomicAdd(T &x, T v) {
  T old = x;
  x = old + v;
  return old;
}
template <class T>
YAKL_INLINE T atomicMin(T &x, T v) {
  T old = x;
  x = std::min(old, v);
  return old;
}
template <class T>
YAKL_INLINE T atomicMax(T &x, T v) {
  T old = x;
  x = std::max(old, v);
  return old;
}

// ---------------------------------------------------------------------------------------------------------------------
namespace c {

struct LBnd {
  int l, u;   // inclusive
  LBnd(int n) : l(0), u(n - 1) {}
  LBnd(int lo, int hi) : l(lo), u(hi) {}
  LBnd(std::initializer_list<int> b) {
    if (b.size() != 2) yakl_throw("yakl stand-in: a bound is {lower, upper}");
    l = *b.begin();
    u = *(b.begin() + 1);
  }
};

template <int N>
struct Bounds {
  int lo[N], hi[N];   // inclusive
  template <class... B, typename std::enable_if<sizeof...(B) == N, int>::type = 0>
  Bounds(B... b) {
    LBnd bb[N] = {LBnd(b)...};
    for (int i = 0; i < N; i++) {
      lo[i] = bb[i].l;
      hi[i] = bb[i].u;
    }
  }
};

template <int N>
struct SimpleBounds {
  int hi[N];   // exclusive, lower bound 0
  template <class... B, typename std::enable_if<sizeof...(B) == N, int>::type = 0>
  SimpleBounds(B... b) : hi{int(b)...} {}
};

namespace detail {
template <int D, int N, class F, class... I>
inline void loop(int const *lo, int const *hi, F const &f, I... ind) {
  if constexpr (D == N) {
    f(ind...);
  } else {
    for (int i = lo[D]; i <= hi[D]; i++) loop<D + 1, N>(lo, hi, f, ind..., i);
  }
}

inline bool replay_matches(char const *label) {
  std::string const &want = standin_state().replay_label;
  if (want.empty() || label == nullptr) return false;
  std::string got(label);
  if (got.size() < want.size() || got.compare(got.size() - want.size(), want.size(), want) != 0) return false;
  return got.size() == want.size() || got[got.size() - want.size() - 1] == '/';
}

template <int N, class F>
inline void run(char const *label, int const *lo, int const *hi, F const &f) {
  int reps = 1;
  if (replay_matches(label)) {
    reps = 2;
    standin_state().replay_count++;
  }
  for (int r = 0; r < reps; r++) loop<0, N>(lo, hi, f);
}
}  // namespace detail

template <class F>
inline void parallel_for(char const *label, int n, F const &f) {
  int lo[1] = {0}, hi[1] = {n - 1};
  detail::run<1>(label, lo, hi, f);
}
template <int N, class F>
inline void parallel_for(char const *label, SimpleBounds<N> const &b, F const &f) {
  int lo[N], hi[N];
  for (int i = 0; i < N; i++) {
    lo[i] = 0;
    hi[i] = b.hi[i] - 1;
  }
  detail::run<N>(label, lo, hi, f);
}
template <int N, class F>
inline void parallel_for(char const *label, Bounds<N> const &b, F const &f) {
  detail::run<N>(label, b.lo, b.hi, f);
}
template <class B, class F>
inline void parallel_for(std::string const &label, B const &b, F const &f) {
  parallel_for(label.c_str(), b, f);
}
template <class F>
inline void parallel_for(int n, F const &f) {
  parallel_for((char const *)nullptr, n, f);
}
template <int N, class F>
inline void parallel_for(SimpleBounds<N> const &b, F const &f) {
  parallel_for((char const *)nullptr, b, f);
}
template <int N, class F>
inline void parallel_for(Bounds<N> const &b, F const &f) {
  parallel_for((char const *)nullptr, b, f);
}

}  // namespace c

// ---------------------------------------------------------------------------------------------------------------------
namespace intrinsics {

template <class T, int N, int M, int S>
typename std::remove_cv<T>::type minval(Array<T, N, M, S> const &a) {
  typename std::remove_cv<T>::type m = a.myData[0];
  for (size_t i = 1; i < a.totElems(); i++)
    if (a.myData[i] < m) m = a.myData[i];
  return m;
}
template <class T, int N, int M, int S>
typename std::remove_cv<T>::type maxval(Array<T, N, M, S> const &a) {
  typename std::remove_cv<T>::type m = a.myData[0];
  for (size_t i = 1; i < a.totElems(); i++)
    if (a.myData[i] > m) m = a.myData[i];
  return m;
}
template <class T, int N, int M, int S>
typename std::remove_cv<T>::type sum(Array<T, N, M, S> const &a) {
  typename std::remove_cv<T>::type s = 0;
  for (size_t i = 0; i < a.totElems(); i++) s += a.myData[i];
  return s;
}
template <class T, int N, int M, int S>
Array<typename std::remove_cv<T>::type, N, M, S> abs(Array<T, N, M, S> const &a) {
  auto r = a.createDeviceCopy();
  Array<typename std::remove_cv<T>::type, N, M, S> out;
  out.myname = r.myname;
  out.owner = r.owner;
  out.myData = r.myData;
  for (int i = 0; i < N; i++) out.dimension[i] = r.dimension[i];
  for (size_t i = 0; i < out.totElems(); i++) out.myData[i] = std::abs(out.myData[i]);
  return out;
}
template <class T, int N, int M, int S>
size_t size(Array<T, N, M, S> const &a) {
  return a.totElems();
}
template <class T, int N, int M, int S>
int size(Array<T, N, M, S> const &a, int dim) {
  return a.extent(dim);
}

// Gauss-Jordan elimination without pivoting, first index = column.  This is the project's assumption of YAKL's
// algorithm (deviation D3): it stays UNPINNED, oracle and stand-in share it by construction.
template <class T, unsigned n>
SArray<T, 2, n, n> matinv_ge(SArray<T, 2, n, n> const &a) {
  SArray<T, 2, n, n> s, inv;
  for (unsigned c = 0; c < n; c++)
    for (unsigned r = 0; r < n; r++) {
      s(c, r) = a(c, r);
      inv(c, r) = (c == r) ? T(1) : T(0);
    }
  for (unsigned d = 0; d < n; d++) {
    T factor = T(1) / s(d, d);
    for (unsigned c = d; c < n; c++) s(c, d) *= factor;
    for (unsigned c = 0; c < n; c++) inv(c, d) *= factor;
    for (unsigned r = d + 1; r < n; r++) {
      T f = s(d, r);
      for (unsigned c = d; c < n; c++) s(c, r) -= f * s(c, d);
      for (unsigned c = 0; c < n; c++) inv(c, r) -= f * inv(c, d);
    }
  }
  for (int d = int(n) - 1; d >= 1; d--) {
    for (int r = 0; r < d; r++) {
      T f = s(d, r);
      for (unsigned c = r + 1; c < n; c++) s(c, r) -= f * s(c, d);
      for (unsigned c = 0; c < n; c++) inv(c, r) -= f * inv(c, d);
    }
  }
  return inv;
}

}  // namespace intrinsics
}  // namespace yakl
