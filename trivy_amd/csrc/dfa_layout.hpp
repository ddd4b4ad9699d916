// The LDS image of one K2 group DFA: where k2_run stages its tables, and which of the two
// accept layouts the kernels read.  make_device_dfa (kernels.hip) uploads by it; the plan
// introspection hook tsg_ruleset_group_table (capi.cpp) reports it without a device.
//
//   per-state  (state_acc = 1): every transition out of a state carries the same accept-mask
//              index, so the index is kept per state and staged in LDS with the masks;
//   look-ahead (state_acc = 0): the accepts differ per byte class (a trailing empty-width
//              assertion decided by the next byte: $, \b, \B, (?m)$), or the per-state image
//              does not fit: the index is read per transition from global memory.
#pragma once
#include <algorithm>
#include <cstdint>

#include "dfa.hpp"

namespace tsg {

struct DevDfaLayout {
  uint32_t nc = 0;         // row width (byte classes, at least 2: state_of's reciprocal needs it)
  uint32_t o_cls = 0, o_dead = 0, o_accs = 0, o_masks = 0;
  uint32_t state_acc = 0;  // 1: per-state accepts staged in LDS; 0: look-ahead
  uint32_t lds_bytes = 0;
};

inline uint32_t dfa_align16(uint32_t x) { return (x + 15) & ~15u; }

inline DevDfaLayout dev_dfa_layout(const DFA& d) {
  DevDfaLayout v;
  const size_t nc0 = (size_t)d.nclasses;
  v.nc = (uint32_t)std::max<size_t>(nc0, 2);
  bool uniform = true;
  for (int s = 0; s < d.nstates && uniform; s++)
    for (size_t c = 1; c < nc0; c++)
      if (d.acc[(size_t)s * nc0 + c] != d.acc[(size_t)s * nc0]) {
        uniform = false;
        break;
      }
  size_t mask_words = 0;
  for (const auto& m : d.masks) mask_words += m.size();
  uint32_t o = dfa_align16((uint32_t)((size_t)d.nstates * v.nc * 2));
  v.o_cls = o;
  o += 256;
  v.o_dead = o;  // the tails' per-word liveness test reads it
  o += dfa_align16((uint32_t)d.nstates);
  v.o_accs = o;
  v.o_masks = o;
  const uint32_t acc_bytes = dfa_align16((uint32_t)d.nstates * 2) + dfa_align16((uint32_t)mask_words * 8);
  if (uniform && o + acc_bytes + 16 * 1024 <= 150 * 1024) {
    v.state_acc = 1;
    v.o_masks = o + dfa_align16((uint32_t)d.nstates * 2);
    o += acc_bytes;
  }
  v.lds_bytes = o + 16;
  return v;
}

}  // namespace tsg
