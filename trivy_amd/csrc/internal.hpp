// Shared internals of the C ABI (capi.cpp, pipeline.cpp, layer.cpp, multi.cpp, kernels.hip).
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <memory>
#include <mutex>
#include <string>
#include <utility>

#include "../../include/trivy_secret.h"
#include "plan.hpp"
#include "scanner.hpp"

struct tsg_ruleset {
  tsg::Ruleset rs;
  std::unique_ptr<tsg::Plan> plan;
};

struct tsg_result {
  std::string buf;
};

namespace tsg {
void set_error(const std::string& msg);
int fail(int code, const std::string& msg);
// the rule set a context was created with (pipeline.cpp)
const tsg_ruleset* ctx_ruleset(const tsg_ctx* c);
// bytes of a default pinned slot (tsg_ctx_options.slot_mib)
uint64_t ctx_slot_bytes(const tsg_ctx* c);
// utils.IsBinary (utils.go:71-89) of a file of n bytes at p: layer.cpp's is_binary
bool is_binary_head(const uint8_t* p, uint64_t n);


// ---- a layer tar in device memory (tsg_device_layer_scan): layer.cpp drives the walk,
// pipeline.cpp owns the device.  Under TSG_CTX_EMULATE the "device" pointer is a host pointer.
// archive/tar's header checksum test and the all-zero test of one 512-byte block (layer.cpp)
void tar_block_marks(const uint8_t* block, bool* header, bool* zero);
// the two bitmaps of tar_mark_kernel (device.hpp mark_tar) or of their emulation:
// marks[0, words) header bits, marks[words, 2 * words) zero bits, words = (tar_len / 512 + 63) / 64
int ctx_tar_marks(tsg_ctx* c, const void* d_tar, uint64_t tar_len, uint64_t* marks, double* ms);
// A buffer of the context's small pool of pinned, device-visible memory (plain memory when
// emulated); ctx_fetch_ranges grows it.  Given back with ctx_pin_give (reused by later calls).
struct PinBuf {
  uint8_t* p = nullptr;
  uint64_t cap = 0;
};
void ctx_pin_give(tsg_ctx* c, PinBuf* b);
// dst->p = the listed {offset, length} ranges of the base_bytes bytes at d_base, back to back
// in list order (gather_kernel: adjacent ranges merge, segments are cut to kGatherSegBytes;
// memcpy of the same segments when emulated).  Every range lies inside the buffer.
int ctx_fetch_ranges(tsg_ctx* c, const void* d_base, uint64_t base_bytes,
                     const std::pair<uint64_t, uint64_t>* ranges, size_t n, PinBuf* dst);
// tsg_batch_collect of a device-resident batch, and the bytes its fetch brought to the host
int ctx_collect_device(tsg_ctx* c, uint64_t ticket, tsg_result** out, uint64_t* fetched_bytes);
// one finished tsg_device_layer_scan: `last` holds the call's fields; the sums are kept here
void ctx_device_layer_done(tsg_ctx* c, const tsg_device_layer_stats& last);

// test and measurement knobs (knobs.cpp, tsg_test_knob); 0 = default
struct Knobs {
  std::atomic<int64_t> tar_range_kib{0}, piece_mib{0}, pike_only{0}, no_k1x{0}, emu_wordrec{0},
      x_step{0}, k1_automaton{0}, group_states{0}, group_table_kib{0}, k1f_grid{0},
      k1f_list{0}, k2_items_cap{0}, k2_max_dense{0}, k2_no_word_recs{0}, device_poison{0}, grid_cap{0};
  std::mutex m;
  std::string emu_kw_unknown;
};
Knobs& knobs();
std::string knob_kw_unknown();

// A grid whose size comes from the device or from a constant, under the test knob grid_cap
// (cap = its value, read once per batch or call; 0 leaves the grid as computed).  Every such
// kernel walks its work in a loop, so fewer blocks only mean more rounds per block.
inline int capped_grid(uint64_t grid, int64_t cap) {
  return (int)(cap > 0 ? std::min<uint64_t>(grid, (uint64_t)cap) : grid);
}

// K2's item capacity for a batch of nchunks chunks: twice the batch's chunks (the builtin
// rules list ~11 % of them), at least 64 Ki items; and the number of groups the dense pass
// takes.  Past either, groups are skipped and resolved on the host.  (Knobs k2_items_cap /
// k2_max_dense replace them in tests.)
inline uint64_t k2_items_cap(uint64_t nchunks) {
  const int64_t k = knobs().k2_items_cap.load();
  return k > 0 ? (uint64_t)k : std::max<uint64_t>(2 * nchunks, 1u << 16);
}
inline uint32_t k2_max_dense() {
  const int64_t k = knobs().k2_max_dense.load();
  return k > 0 ? (uint32_t)k : 16u;
}
}  // namespace tsg
