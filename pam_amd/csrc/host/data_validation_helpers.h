// data_validation_helpers.h -- the helpers (pam::validation) of DataManager::validate_all / validate / validate_nan / validate_inf /
// validate_pos of the work-alike coupler
// (pam_core/DataManager.h:408-509), on top of pam_amd_validate_fields (include/pam_amd_modules.h).
//
// The reference copies every entry to the host and loops there ("This is EXPENSIVE").  Here the device scans all entries of a call at
// once -- one launch per 32 entries, one synchronisation, 48 bytes back per entry -- and only an entry in which the scan found an
// offender is copied to the host, where the reference's own loops write the reference's lines, character for character and in its
// order: per entry in REGISTRATION order every NaN line, then every inf line, then every negative line; with die_on_failed_check,
// endrun("") after the first line.  A clean state prints nothing and copies nothing but the counts.  Nothing is allocated per entry
// on the device; the host copy of a dirty entry lives for the length of its report.
//
// Checked: double and float entries for NaN and inf; double, float, int and long long entries registered positive-definite for
// negative values.  NOT checked: bool (as in the reference) and short, unsigned and long double entries, which the reference does look
// at and nothing in PAM registers.  The flat index printed is 64-bit (the reference's `int i` wraps past 2^31 elements).  The work runs
// on the default stream, like the modules.
//
// pam_coupler.h includes this file above the DataManager; the five members themselves, which the class only declares, are defined in
// data_validation_members.h, which it includes below the coupler.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <iostream>
#include <string>
#include <type_traits>
#include <vector>

#include "pam_amd_awfl.h"
#include "pam_amd_modules.h"

namespace pam {
namespace validation {

// the `kind` of pam_amd_validate_fields for an entry of type T; -1: the entry is not checked
template <class T>
constexpr int kind_of() {
  typedef typename std::remove_cv<T>::type U;
  return std::is_same<U, double>::value ? 0
       : std::is_same<U, float>::value ? 1
       : std::is_same<U, int>::value ? 2
       : (std::is_same<U, long long>::value || (std::is_same<U, long>::value && sizeof(long) == 8)) ? 3
       : -1;
}

constexpr unsigned CHECK_NAN = 1u, CHECK_INF = 2u, CHECK_POS = 4u, CHECK_ALL = 7u;

// one entry of a check: what the members hand over (the DataManager's Entry is private to it)
struct Item {
  std::string name;
  int kind;
  void const *ptr;
  long long size;
  bool positive;
  size_t seq;   // registration sequence number of the entry
};

// DataManager.h:471-509: the three loops over the host copy, each line followed by endrun("") where `die` is set
template <class T>
inline void report_loops(std::string const &name, T const *arr, long long n, bool positive, unsigned which, bool die) {
  if ((which & CHECK_NAN) && std::is_floating_point<T>::value)
    for (long long i = 0; i < n; i++)
      if (std::isnan((double)arr[i])) {
        std::cerr << "WARNING: NaN discovered in: " << name << " at global index: " << i << "\n";
        if (die) endrun("");
      }
  if ((which & CHECK_INF) && std::is_floating_point<T>::value)
    for (long long i = 0; i < n; i++)
      if (std::isinf((double)arr[i])) {
        std::cerr << "WARNING: inf discovered in: " << name << " at global index: " << i << "\n";
        if (die) endrun("");
      }
  if ((which & CHECK_POS) && positive)
    for (long long i = 0; i < n; i++)
      if (arr[i] < 0.) {
        std::cerr << "WARNING: negative value discovered in positive-definite entry: " << name << " at global index: " << i << "\n";
        if (die) endrun("");
      }
}

// an entry the scan found offenders in: copied to the host once, then the reference's loops
inline void report(Item const &it, unsigned which, bool die) {
  const size_t bytes = (size_t)it.size * ((it.kind == 0 || it.kind == 3) ? 8 : 4);
  std::vector<char> host(bytes);
  if (hipMemcpy(host.data(), it.ptr, bytes, hipMemcpyDeviceToHost) != hipSuccess)
    endrun("ERROR: validate: could not copy entry " + it.name + " to the host");
  switch (it.kind) {
    case 0: report_loops(it.name, (double const *)host.data(), it.size, it.positive, which, die); break;
    case 1: report_loops(it.name, (float const *)host.data(), it.size, it.positive, which, die); break;
    case 2: report_loops(it.name, (int const *)host.data(), it.size, it.positive, which, die); break;
    default: report_loops(it.name, (long long const *)host.data(), it.size, it.positive, which, die); break;
  }
}

// the whole check of a list of entries (registration order): one device scan, then the reports of the dirty ones.  `which` selects
// the classes reported (validate_nan / validate_inf / validate_pos look at one each).
inline void check(std::vector<Item> const &items, unsigned which, bool die) {
  if (items.empty()) return;
  const size_t n = items.size();
  std::vector<int> kind(n), positive(n);
  std::vector<long long> size(n), count(3 * n), first(3 * n);
  std::vector<void const *> data(n);
  for (size_t f = 0; f < n; f++) {
    kind[f] = items[f].kind;
    size[f] = items[f].size;
    data[f] = items[f].ptr;
    positive[f] = items[f].positive ? 1 : 0;
  }
  if (pam_amd_validate_fields((int)n, kind.data(), size.data(), data.data(), positive.data(), count.data(), first.data(), nullptr))
    endrun(pam_amd_awfl_last_error());
  for (size_t f = 0; f < n; f++) {
    const bool dirty = ((which & CHECK_NAN) && count[3 * f]) || ((which & CHECK_INF) && count[3 * f + 1]) ||
                       ((which & CHECK_POS) && count[3 * f + 2]);
    if (dirty) report(items[f], which, die);
  }
}

}  // namespace validation
}  // namespace pam
