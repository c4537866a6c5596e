// data_diagnostics.h -- what the state LOOKS like, taken on the device: DataManager::diagnose / diagnose_all of the work-alike coupler
// and the reference's DEBUG_PRINT_SUM / AVG / MIN / MAX(var) (pam_core/pam_const.h:308-333) for the work-alike's arrays, on top of
// pam_amd_field_diagnostics (include/pam_amd_modules.h).  The companion of DataManager::validate (data_validation_*.h), which answers
// whether the state is broken.
//
// The reference's macros call yakl::intrinsics::sum / minval / maxval and print one line to std::cout; a host model that wants the
// numbers of an ensemble copies the arrays to the host.  Here the device reads all entries of a call once -- two launches per 32 entries,
// one synchronisation, 48 bytes back per result -- and returns per entry, or per ensemble MEMBER of an entry (the member is the fastest
// axis of every coupler array), the least and the greatest element with their flat indices, the number of NaNs and the sum.  diagnose and
// diagnose_all return structs and print nothing.
//
// THE SUM.  vsum is the IEEE double sum by the fixed tree of pam_amd_modules.h: the same bits from run to run, on every device and however
// an ensemble is cut into member chunks.  The reference's sum is yakl::intrinsics::sum, whose order is YAKL's own and is not pinned
// (it differs between YAKL's back ends), so the two agree NOT bit for bit but to the bound of a summation tree: each is within
// gamma_D sum|x| of the exact sum, gamma_D = D u / (1 - D u), u = 2^-53, D the adds on an element's path (here 15 per level for a whole
// field, 65 per member).  minval and maxval are exact and agree exactly.  The macros print the reference's lines, character for character, with the stream's default precision as there.
//
// Looked at: double and float entries.  Every other type is skipped by diagnose_all and refused by diagnose; with members = M, so is an
// entry whose size is no multiple of M.  The work runs on the default stream, like the modules.
//
// pam_coupler.h includes this file below the coupler, after the validation members.
#pragma once
#include <algorithm>
#include <cmath>
#include <iostream>
#include <string>
#include <vector>

#include "pam_amd_awfl.h"
#include "pam_amd_modules.h"

namespace pam {
namespace diagnostics {

// one entry (members = 0: one result, index 0) or its M members
struct FieldDiagnostics {
  std::string name;
  long long size = 0;   // elements of the entry
  int members = 0;
  std::vector<double> vmin, vmax, vsum;               // NaNs take no part in vmin / vmax; +inf / -inf where every element is a NaN
  std::vector<long long> argmin, argmax, nan_count;   // flat indices into the entry, the lowest among equal values; -1: every element a NaN
  double max_abs(size_t m = 0) const { return std::max(-vmin[m], vmax[m]); }
  double mean(size_t m = 0) const { return vsum[m] / (double)(size / std::max(members, 1)); }
};

struct Item {
  std::string name;
  int kind;   // 0 double, 1 float
  void const *ptr;
  long long size;
  size_t seq;
};

// one device scan of a list of entries
inline std::vector<FieldDiagnostics> scan(std::vector<Item> const &items, int members = 0) {
  std::vector<FieldDiagnostics> out(items.size());
  if (items.empty()) return out;
  const size_t n = items.size(), M = (size_t)std::max(members, 1);
  std::vector<int> kind(n);
  std::vector<long long> size(n), argmin(n * M), argmax(n * M), nans(n * M);
  std::vector<void const *> data(n);
  std::vector<double> vmin(n * M), vmax(n * M), vsum(n * M);
  for (size_t f = 0; f < n; f++) {
    kind[f] = items[f].kind;
    size[f] = items[f].size;
    data[f] = items[f].ptr;
  }
  if (pam_amd_field_diagnostics((int)n, kind.data(), size.data(), data.data(), members, vmin.data(), vmax.data(), vsum.data(),
                                argmin.data(), argmax.data(), nans.data(), nullptr))
    endrun(pam_amd_awfl_last_error());
  for (size_t f = 0; f < n; f++) {
    FieldDiagnostics &d = out[f];
    d.name = items[f].name;
    d.size = items[f].size;
    d.members = members;
    d.vmin.assign(vmin.begin() + f * M, vmin.begin() + (f + 1) * M);
    d.vmax.assign(vmax.begin() + f * M, vmax.begin() + (f + 1) * M);
    d.vsum.assign(vsum.begin() + f * M, vsum.begin() + (f + 1) * M);
    d.argmin.assign(argmin.begin() + f * M, argmin.begin() + (f + 1) * M);
    d.argmax.assign(argmax.begin() + f * M, argmax.begin() + (f + 1) * M);
    d.nan_count.assign(nans.begin() + f * M, nans.begin() + (f + 1) * M);
  }
  return out;
}

// a work-alike array (DeviceView<double>, DeviceView<float const>, ...) as a list of one
template <class VIEW>
inline FieldDiagnostics of_array(VIEW const &var, char const *varname) {
  const int kind = validation::kind_of<typename std::remove_pointer<decltype(var.data())>::type>();
  if (kind != 0 && kind != 1) endrun(std::string("ERROR: diagnostics: not a double or float array: ") + varname);
  if (var.size() < 1) endrun(std::string("ERROR: diagnostics: empty array: ") + varname);
  return scan({Item{varname, kind, (void const *)var.data(), (long long)var.size(), 0}})[0];
}

}  // namespace diagnostics

// every double and float entry, in registration order
inline std::vector<diagnostics::FieldDiagnostics> DataManager::diagnose_all(int members) const {
  std::vector<diagnostics::Item> items;
  for (auto const &e : entries) {
    long long n = 1;
    for (int d : e.second.dims) n *= d;
    if ((e.second.kind == 0 || e.second.kind == 1) && n >= 1 && n % std::max(members, 1) == 0)
      items.push_back({e.first, e.second.kind, e.second.ptr, n, e.second.seq});
  }
  std::sort(items.begin(), items.end(), [](diagnostics::Item const &a, diagnostics::Item const &b) { return a.seq < b.seq; });
  return diagnostics::scan(items, members);
}

inline diagnostics::FieldDiagnostics DataManager::diagnose(std::string name, int members) const {
  auto it = entries.find(name);
  if (it == entries.end()) endrun("ERROR: Could not find entry " + name);
  long long n = 1;
  for (int d : it->second.dims) n *= d;
  if (it->second.kind != 0 && it->second.kind != 1) endrun("ERROR: diagnose: entry " + name + " is neither double nor float");
  if (n < 1 || n % std::max(members, 1) != 0) endrun("ERROR: diagnose: the size of entry " + name + " is no multiple of members");
  return diagnostics::scan({diagnostics::Item{name, it->second.kind, it->second.ptr, n, it->second.seq}}, members)[0];
}

}  // namespace pam

// pam_const.h:308-322: the lines of debug_print_sum / avg / min / max, character for character.  minval and maxval print in the array's
// own type, as there (a float through a double prints the same digits).
inline void debug_print_line(char const *file, int line, char const *what, char const *varname, double value) {
  std::cout << "*** DEBUG: " << file << ": " << line << ": " << what << "(" << varname << ")  -->  " << value << std::endl;
}
#define DEBUG_PRINT_SUM(var) { debug_print_line(__FILE__, __LINE__, "sum", #var, pam::diagnostics::of_array((var), #var).vsum[0]); }
#define DEBUG_PRINT_AVG(var) { debug_print_line(__FILE__, __LINE__, "avg", #var, pam::diagnostics::of_array((var), #var).mean()); }
#define DEBUG_PRINT_MIN(var) { debug_print_line(__FILE__, __LINE__, "minval", #var, pam::diagnostics::of_array((var), #var).vmin[0]); }
#define DEBUG_PRINT_MAX(var) { debug_print_line(__FILE__, __LINE__, "maxval", #var, pam::diagnostics::of_array((var), #var).vmax[0]); }
