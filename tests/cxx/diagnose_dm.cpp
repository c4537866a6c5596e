// diagnose_dm.cpp -- the work-alike DataManager's diagnostics (pam_amd/csrc/host/pam_coupler.h, data_diagnostics.h) driven from a script.
// TEST INFRASTRUCTURE ONLY: tests/test_diagnostics.py builds it with hipcc the way the examples' driver is built.  The script (argv[1])
// has one command per line:
//   entry NAME KIND N HEX...   register_and_allocate<KIND>(NAME, ...) and fill it with the N bit patterns (KIND: double, float, int)
//   macros NAME KIND           DEBUG_PRINT_SUM / AVG / MIN / MAX of the entry's array: the reference's four lines on stdout
//   diagnose NAME M            "### NAME M" and per result "vmin vmax vsum argmin argmax nan_count" (the doubles as %a), "###END"
//   diagnose_all M             the same for every entry diagnose_all returns, in its order
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "pam_coupler.h"

template <class T, class U>
static void add(pam::DataManager &dm, std::string const &name, std::vector<unsigned long long> const &bits) {
  dm.register_and_allocate<T>(name, "", {(int)bits.size()}, {"dim_" + name});
  std::vector<U> host(bits.size());
  for (size_t i = 0; i < bits.size(); i++) host[i] = (U)bits[i];
  static_assert(sizeof(T) == sizeof(U), "bit patterns of the element's size");
  auto view = dm.get_collapsed<T>(name);
  if (hipMemcpy(view.data(), host.data(), host.size() * sizeof(U), hipMemcpyHostToDevice) != hipSuccess) endrun("copy failed");
}

template <class T>
static void macros(pam::DataManager &dm, std::string const &name) {
  auto var = dm.get_collapsed<T>(name);
  DEBUG_PRINT_SUM(var)
  DEBUG_PRINT_AVG(var)
  DEBUG_PRINT_MIN(var)
  DEBUG_PRINT_MAX(var)
}

static void show(pam::diagnostics::FieldDiagnostics const &d) {
  std::printf("### %s %d\n", d.name.c_str(), d.members);
  for (size_t m = 0; m < d.vmin.size(); m++)
    std::printf("%a %a %a %lld %lld %lld\n", d.vmin[m], d.vmax[m], d.vsum[m], d.argmin[m], d.argmax[m], d.nan_count[m]);
  std::printf("###END\n");
  std::fflush(stdout);
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  pam::DataManager dm;
  std::string line;
  try {
    while (std::getline(in, line)) {
      std::istringstream ss(line);
      std::string cmd, name, kind;
      ss >> cmd;
      if (cmd == "entry") {
        size_t n;
        ss >> name >> kind >> n;
        std::vector<unsigned long long> bits(n);
        for (auto &b : bits) ss >> std::hex >> b;
        if (kind == "double") add<double, uint64_t>(dm, name, bits);
        else if (kind == "float") add<float, uint32_t>(dm, name, bits);
        else if (kind == "int") add<int, uint32_t>(dm, name, bits);
        else return 3;
      } else if (cmd == "macros") {
        ss >> name >> kind;
        std::cout.flush();
        if (kind == "double") macros<double>(dm, name);
        else if (kind == "float") macros<float>(dm, name);
        else return 3;
      } else if (cmd == "diagnose") {
        int members;
        ss >> name >> members;
        pam::DataManager const &cdm = dm;
        show(cdm.diagnose(name, members));
      } else if (cmd == "diagnose_all") {
        int members;
        ss >> members;
        pam::DataManager const &cdm = dm;
        for (auto const &d : cdm.diagnose_all(members)) show(d);
      } else if (!cmd.empty()) {
        return 5;
      }
    }
  } catch (std::string const &msg) {
    std::printf("### threw %s\n", msg.c_str());
  }
  dm.finalize();
  pam_amd_modules_finalize();
  return 0;
}
