// C entry points around the reference's own pam_core/DataManager.h, compiled serially against the YAKL stand-in (oracle/ref/YAKL.h).
// TEST INFRASTRUCTURE ONLY: tests/golden/make_ref_validate_golden.py builds it in a temporary directory, registers the entries of a
// case, calls validate / validate_all and records what they wrote to std::cerr in tests/golden/validate_ref.json; nothing compiled is
// kept.  Every entry is one-dimensional with a dimension name of its own.
#define YAKL_STANDIN_DEFINE_GLOBALS
#include "YAKL.h"

#include "DataManager.h"

#include <cstring>
#include <iostream>
#include <mutex>
#include <sstream>
#include <string>

namespace pam {
std::mutex data_manager_mutex;
}

namespace {
template <class T>
void add(pam::DataManager &dm, std::string name, long long n, void const *src, bool positive) {
  dm.register_and_allocate<T>(name, "", {(int)n}, {"dim_" + name}, positive);
  auto a = dm.get_collapsed<T>(name);
  std::memcpy(a.data(), src, (size_t)n * sizeof(T));
}
}  // namespace

extern "C" {

void *rv_new() { return new pam::DataManager(); }
void rv_free(void *dm) { delete (pam::DataManager *)dm; }

// kind: 0 double, 1 float, 2 int, 3 long long, 4 bool (one byte per element); src: the elements' bytes
int rv_register(void *dm_, char const *name, int kind, long long n, void const *src, int positive) {
  auto &dm = *(pam::DataManager *)dm_;
  try {
    switch (kind) {
      case 0: add<double>(dm, name, n, src, positive != 0); break;
      case 1: add<float>(dm, name, n, src, positive != 0); break;
      case 2: add<int>(dm, name, n, src, positive != 0); break;
      case 3: add<long long>(dm, name, n, src, positive != 0); break;
      case 4: add<bool>(dm, name, n, src, positive != 0); break;
      default: return -2;
    }
    return 0;
  } catch (...) {
    return -1;
  }
}

// name == NULL: validate_all(die); otherwise validate(name, die).  What went to std::cerr is copied to out (at most cap - 1 bytes);
// returns 1 where the call ended in endrun's throw, 0 where it returned, -1 for any other exception, -2 where out is too small.
int rv_call(void *dm_, char const *name, int die, char *out, int cap) {
  auto const &dm = *(pam::DataManager const *)dm_;
  std::ostringstream text;
  std::streambuf *old = std::cerr.rdbuf(text.rdbuf());
  int rc = 0;
  try {
    if (name) dm.validate(name, die != 0);
    else dm.validate_all(die != 0);
  } catch (std::string const &) {
    rc = 1;
  } catch (...) {
    rc = -1;
  }
  std::cerr.rdbuf(old);
  std::string s = text.str();
  if ((int)s.size() >= cap) return -2;
  std::memcpy(out, s.c_str(), s.size() + 1);
  return rc;
}

}  // extern "C"
