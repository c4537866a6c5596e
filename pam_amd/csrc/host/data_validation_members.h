// data_validation_members.h -- the definitions of DataManager::validate_all / validate / validate_nan / validate_inf / validate_pos
// (pam_core/DataManager.h:408-509), which the work-alike's class only declares.  pam_coupler.h includes this file below the coupler; the
// helpers and the description of the check are in data_validation_helpers.h.
#pragma once
#include <algorithm>

namespace pam {

// DataManager.h:411-413: every entry, in registration order (the map is alphabetical: the sequence numbers restore the order)
inline void DataManager::validate_all(bool die_on_failed_check) const {
  std::vector<validation::Item> items;
  for (auto const &e : entries) {
    long long n = 1;
    for (int d : e.second.dims) n *= d;
    if (e.second.kind >= 0 && n >= 1) items.push_back({e.first, e.second.kind, e.second.ptr, n, e.second.positive, e.second.seq});
  }
  std::sort(items.begin(), items.end(), [](validation::Item const &a, validation::Item const &b) { return a.seq < b.seq; });
  validation::check(items, validation::CHECK_ALL, die_on_failed_check);
}

namespace validation {
// one named entry as a list of at most one Item (an unchecked type or an empty entry: nothing to look at)
template <class ENTRIES>
inline std::vector<Item> one_item(ENTRIES const &entries, std::string const &name) {
  auto it = entries.find(name);
  if (it == entries.end()) endrun("ERROR: Could not find entry " + name);
  long long n = 1;
  for (int d : it->second.dims) n *= d;
  std::vector<Item> items;
  if (it->second.kind >= 0 && n >= 1) items.push_back({name, it->second.kind, it->second.ptr, n, it->second.positive, it->second.seq});
  return items;
}
}  // namespace validation

// DataManager.h:419-423
inline void DataManager::validate(std::string name, bool die_on_failed_check) const {
  validation::check(validation::one_item(entries, name), validation::CHECK_ALL, die_on_failed_check);
}

// DataManager.h:428-466
inline void DataManager::validate_nan(std::string name, bool die_on_failed_check) const {
  validation::check(validation::one_item(entries, name), validation::CHECK_NAN, die_on_failed_check);
}
inline void DataManager::validate_inf(std::string name, bool die_on_failed_check) const {
  validation::check(validation::one_item(entries, name), validation::CHECK_INF, die_on_failed_check);
}
inline void DataManager::validate_pos(std::string name, bool die_on_failed_check) const {
  validation::check(validation::one_item(entries, name), validation::CHECK_POS, die_on_failed_check);
}

}  // namespace pam
