// YAKL.h -- what physics/sgs/shoc/SGS.h needs beyond the YAKL stand-in of oracle/ref/YAKL.h, supplied WITHOUT touching either: the
// reference writes `a.reshape<2>({n0,n1})` (rank as a template argument, extents as a braced list; SGS.h:262-266), the stand-in has
// only `a.reshape(n0, n1)`.  TEST INFRASTRUCTURE ONLY, found before oracle/ref on the include path of tests/ref_shoc/harness.cpp.
// The member is added to the stand-in's Array while its text is read: the token `get_rank()` of its one-line member
// `int get_rank() const { return N; }` expands to that member, the new one, and the head of a second, unused one-liner.
#pragma once
#include <initializer_list>
#define get_rank()                                                                                                      \
  get_rank() const { return N; }                                                                                        \
  template <int M_>                                                                                                     \
  Array<T, M_, MEM, STYLE> reshape(std::initializer_list<int> dims_) const {                                            \
    Array<T, M_, MEM, STYLE> r(myname, myData, std::vector<int>(dims_));                                                \
    if (r.totElems() != totElems()) yakl_throw("yakl stand-in: reshape changes the element count");                      \
    r.owner = owner;                                                                                                    \
    return r;                                                                                                           \
  }                                                                                                                     \
  int get_rank_of_the_standin_()
#include "../../oracle/ref/YAKL.h"
#undef get_rank
