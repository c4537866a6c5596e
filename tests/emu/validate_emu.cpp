// validate_emu.cpp -- HOST EMULATION of the state check's device bodies (pam_amd/csrc/validate_device.h, compiled with g++).  TEST
// INFRASTRUCTURE ONLY (never shipped, never linked into libpam_amd_awfl.so).  The grid of validate_kernel (modules_kernels.hip) is walked
// serially: every workgroup's threads run thread_scan, their tallies are folded with tally_merge, and a workgroup that found something
// adds its counts to the field's and takes the minimum of the first indices -- what the kernel's atomics do.
#include "../../pam_amd/csrc/validate_device.h"

using namespace pama::validate;

extern "C" {

// out[6]: count[3], first[3] (-1 where nothing was found); nblocks <= 0: as many workgroups as the field can keep busy.
// Returns the number of workgroups that would have issued atomics.
long long emu_validate(int kind, long long n, const void *data, int positive, long long nblocks, long long *out) {
  if (nblocks <= 0) nblocks = blocks_needed(kind, n);
  Tally field;
  tally_clear(field);
  long long touched = 0;
  for (long long b = 0; b < nblocks; b++) {
    Tally group;
    tally_clear(group);
    for (int tid = 0; tid < THREADS; tid++) {
      Tally t;
      tally_clear(t);
      thread_scan_kind(kind, data, n, positive != 0, b, nblocks, tid, t);
      tally_merge(group, t);
    }
    if (tally_any(group)) {
      touched++;
      tally_merge(field, group);
    }
  }
  for (int c = 0; c < NUM_CLASSES; c++) {
    out[c] = field.count[c];
    out[3 + c] = field.count[c] ? field.first[c] : -1;
  }
  return touched;
}

}
