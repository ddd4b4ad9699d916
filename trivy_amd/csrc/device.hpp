// Host interface of the gfx950 kernels (kernels.hip) for the batch pipeline (pipeline.cpp).
//
// One DeviceRules per device holds the compiled rule set's tables in HBM (K1 literal
// automaton, K2 rule-group DFAs, the Global.AllowPath DFA, gates).  A batch runs on one
// LaneState (its own HIP stream and HBM buffers, each an owning DevBuf grown on demand);
// enqueue_scan computes the batch's shape once (BatchShape), reserves the lane's buffers and
// puts the whole device part of the batch on that stream with no host round trip, stage by
// stage with a BatchEvent recorded before each:
//
//   input     the content by the batch's ScanSource (H2D from the pinned slot; stage_kernel,
//             caller's HBM -> lane buffer; gather_kernel for files given as spans of the
//             caller's buffer) and one H2D of the file offsets
//   prep      zero fills, coarse file map
//   K1        K1F or the keyword automaton (each adapts once), then K1X
//   gates     keyword gates and event-chunk compaction, item counts, item layout
//             (device-side), item lists
//   K2        list pass, dense pass
//   outputs   candidates, keyword bits, overflow / skip flags, counters: written straight
//             into pinned, host-mapped memory
//
// and records the batch's completion event.  Two lanes per device let the H2D of one batch
// overlap the kernels of the other.  The files of a device-resident batch that the host
// resolver reads come to the pinned slot afterwards, on the context's fetch stream
// (DeviceFetch): fetch_kernel (gather_kernel for spans), or one runtime D2H when every file of
// a packed batch is needed.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <memory>
#include <vector>

#include "plan.hpp"

namespace tsg {

struct DeviceRules;

// Stage boundaries of a batch on its lane's stream (HostOut::ev), each named for the stage
// that starts there: the content into the lane buffer (H2D, stage_kernel or gather_kernel) |
// the file offsets' H2D | prep | the wait for the previous batch's kernels (the other
// lane's) | K1 | gates and the item passes | K2 | outputs.  enqueue_scan records them in this
// order and batch_times reads the span from each to the next; kEvDone completes the batch.
enum BatchEvent : int { kEvH2D = 0, kEvMeta, kEvPrep, kEvWait, kEvK1, kEvGates, kEvK2, kEvOut, kEvDone };

// Pinned host memory of one batch's device outputs, which the outputs kernel writes straight
// into host-mapped memory (no runtime D2H copy).
struct HostOut {
  uint8_t* blk = nullptr;       // host-mapped block: counts | gskip | ovf | kw
  uint8_t* blk_dev = nullptr;   // its device address
  uint32_t* kw = nullptr;       // [files_cap * kw_words]
  uint8_t* ovf = nullptr;       // [files_cap] 1 = resolve the file whole
  uint8_t* gskip = nullptr;     // [groups] 1 = K2 skipped the group (item capacity)
  Candidate* cand = nullptr;    // [cand_cap] host-mapped: K2 candidates copied out
  Candidate* cand_dev = nullptr;  // device address of `cand`
  uint32_t* counts = nullptr;   // [kCounts] the batch's counter block (CountSlot)
  uint32_t files_cap = 0, cand_cap = 0, groups = 0, kw_words = 0;
  uint32_t wall_khz = 0;        // the device wall clock's rate (hipDeviceAttributeWallClockRate)
  hipEvent_t ev[kEvDone + 1] = {};  // the batch's stage boundaries (BatchEvent)
};

// The per-batch counter block: u32 slots in HBM (LaneState::counts; prep zeroes them, the
// kernels count into them) which the outputs kernel copies whole to HostOut::counts.  This
// enumeration is the only place the layout is written: the kernels get pointers to their
// slots, the host names every slot it reads.
enum CountSlot : uint32_t {
  kCntCand = 0,          // candidate records K2 reserved (past cand_cap: dropped, file flagged)
  kCntEvChunks = 1,      // event chunks listed (the length of the event list)
  kCntListEntries = 2,   // K2 list entries of the work list (K2Args::nentries)
  kCntDenseEntries = 3,  // K2 dense entries (K2Args::ndentries)
  kCntLayout = 4,        // base of LayoutArgs::stats; its slots are kCntLayout + LayoutStat
  kCntItems = 5,         // items the layout placed (tsg_stats k2_items)
  kCntEntries = 6,       // list entries the layout wrote (k2_launches)
  kCntSkipped = 7,       // groups K2 skipped (groups_skipped)
  kCntK2Diag = 8,        // [4] K2Args::diag (TSG_K2_DIAG): tail bytes, longest tail, tails
                         // over 4 KiB, word replays
  kCntK2Claim = 12,      // [2] K2Args::claim: next list entry, next dense entry
  kCntK1X = 14,          // [2] K1XArgs::stats: records listed, words verified inline
  kCntK1F = 16,          // [2] K1FArgs::stats: words listed, verified arrivals
  kCntK1FSample = 24,    // [2] the same pair of the K1F adaptation's sampling launch
  kCntClk = 32,          // [kClkStamps] u64 device wall-clock stamps (ClkStamp)
  kCounts = 48,
};
enum LayoutStat : uint32_t { kLayItems = 1, kLayEntries = 2, kLaySkipped = 3 };  // LayoutArgs::stats[...]
// The kernels' own spans beside the HIP events around their launches (batch_times).  A
// start is the atomicMax of the clock's complement (= the minimum) over the first blocks.
enum ClkStamp : uint32_t { kClkK1FStart = 0, kClkK1FEnd = 1, kClkGatesStart = 2, kClkK2End = 3, kClkStamps = 4 };
static_assert(kCntDenseEntries < kCntLayout && kCntLayout + kLayItems == kCntItems &&
                  kCntLayout + kLayEntries == kCntEntries && kCntLayout + kLaySkipped == kCntSkipped,
              "the layout's stats are slots 5..7");
static_assert(kCntSkipped < kCntK2Diag && kCntK2Diag + 4 <= kCntK2Claim && kCntK2Claim + 2 <= kCntK1X &&
                  kCntK1X + 2 <= kCntK1F && kCntK1F + 2 <= kCntK1FSample && kCntK1FSample + 2 <= kCntClk,
              "counter ranges overlap");
static_assert(kCntClk % 2 == 0 && kCntClk + 2 * kClkStamps <= kCounts, "clock stamps: 8-byte aligned, inside the block");

// per-batch K2 diagnostics (K2 work that is not the chunks themselves)
struct K2Diag {
  unsigned long long tail_bytes, tail_max, long_tails, replays;
};

// A segment of a gather (gather_kernel): `len` bytes at offset `src` of the caller's buffer
// go to offset `dst` of the destination.  The host lists them (files merged only where they
// are adjacent in both buffers, each cut to kGatherSegBytes).
struct GatherSeg {
  uint64_t src, dst, len;
};

// Where a batch's content comes from.  The offsets always come from pinned host memory.
enum class ScanSource {
  kHostSlot,   // pinned host: one H2D (two when the slot has no room behind the batch)
  kPackedHbm,  // the packed batch in the caller's HBM (tsg_device_submit): stage_kernel
  kHbmSpans,   // files as spans of the caller's HBM buffer (tsg_device_spans_submit): gather_kernel
};

struct ScanInput {
  ScanSource kind;
  const uint64_t* off;       // [nfiles + 1], pinned host
  uint32_t nfiles;
  uint64_t total;
  // kHostSlot: `total` bytes of pinned host memory.  `room` is the slot's whole pinned data
  // buffer (data == room), or null: enqueue_scan writes the zero tail and a copy of the
  // offsets behind the batch there, so one H2D carries all three
  const uint8_t* data = nullptr;
  uint8_t* room = nullptr;
  uint64_t room_bytes = 0;
  // kPackedHbm: `total` bytes in the caller's HBM at any byte alignment, staged into the lane
  // buffer by stage_kernel instead of the content H2D (the pinned slot holds no content
  // until the batch's fetch).  kHbmSpans: the caller's buffer of src_bytes bytes
  const uint8_t* dev_src = nullptr;
  uint64_t src_bytes = 0;
  // kHbmSpans: gather_kernel copies these segments of dev_src into the lane buffer in the
  // stage's place (ngather may be 0).  They lie in pinned memory that outlives the batch's
  // kernels; gather_dev is its device address.
  const GatherSeg* gather = nullptr;
  const GatherSeg* gather_dev = nullptr;
  uint32_t ngather = 0;
};

// pinned bytes a slot's data buffer keeps past its capacity for that tail and the offsets
inline uint64_t slot_room_bytes(uint32_t files_cap) { return (128u << 10) + 8ull * ((uint64_t)files_cap + 1) + 64; }

struct ScanTimes {  // HIP-event milliseconds of one batch on its lane
  float h2d = 0, meta = 0, wait = 0, prep = 0, k1 = 0, gates = 0, k2 = 0, out = 0;
  // device wall clock (stamped inside the kernels): K1F's first block start to last block
  // end; K1F start to K2's last block end; the gates pass's start to K2's end
  float k1_clk = 0, chain_clk = 0, post_k1_clk = 0;
};

struct LaneState;  // HBM buffers + stream + events of one lane

int device_rules_create(int device, const Plan& plan, uint32_t chunk, uint32_t ext_cap,
                        uint32_t adapt_mib, DeviceRules** out);
void device_rules_destroy(DeviceRules* d);
// keyword bits K1 no longer reports after its adaptation (null before / without it)
std::shared_ptr<const std::vector<uint8_t>> device_rules_kw_unknown(const DeviceRules* d);
uint32_t device_rules_hot_states(const DeviceRules* d);
// What the K1 adaptation decided (test hook, tsg_test_adaptation): copies, read under the
// context lock; the gates and events are read back from HBM.  Before an adaptation: adapted
// false, the gates and events the static ones, hits and quiet empty.  hits / quiet ([n_lit],
// by plan literal id) exist on the K1F path only: the automaton's counters are per state,
// not per literal.
struct AdaptationView {
  bool adapted = false, k1_filter = false;
  uint32_t hot_states = 0, ev_hot = 0;
  uint64_t sample_bytes = 0;
  std::vector<uint8_t> kw_unknown;        // [n_kw], zeros before an adaptation
  std::vector<uint8_t> gate_open;         // [G] d_galways
  std::vector<uint8_t> event_everywhere;  // [G] d_gevents & kEvAlways
  std::vector<uint32_t> hits;             // K1F: the sampling launch's counter per literal id
  std::vector<uint8_t> quiet;             // K1F: the literals that left the filter
};
int device_rules_adaptation(const DeviceRules* d, AdaptationView* out);
// true: K1 runs as K1F (k1f_kernel, batches under 4 GiB); false: the automaton (k1_kernel)
bool device_rules_k1_filter(const DeviceRules* d);
// The automaton K1's layout (test hooks tsg_test_k1_layout_of / tsg_test_k1_layout): host
// values only, no device call.  threads = 0: no kernel is built for the layout.
struct K1LayoutView {
  uint32_t packed = 0, states = 0, classes = 0, stride = 0, row_unit = 0, table_bytes = 0;
  uint32_t lds_class = 0, rep = 0, lds_kib = 0, threads = 0, blocks_per_cu = 0, kw_words = 0;
};
// the layout make_device_k1 gives an automaton of ns states and nc classes; TSG_ERR_ARG
// where it (or k1_tables) fails, `out` filled as far as the arithmetic goes
int k1_layout_of(uint32_t ns, uint32_t nc, K1LayoutView* out);
// the same read from the device tables (classes: the plan's)
void device_rules_k1_layout(const DeviceRules* d, K1LayoutView* out);
// true: K2's list pass runs k2_kernel_rich (decided by the occupancy API), false: k2_kernel
bool device_rules_k2_rich(const DeviceRules* d);
// bytes of K1X's verify image (staged in LDS up to kXImgLds), 0 without K1X
uint32_t device_rules_k1x_img_bytes(const DeviceRules* d);

int lane_create(DeviceRules* d, LaneState** out);
void lane_destroy(LaneState* l);
hipStream_t lane_stream(LaneState* l);

// cand_cap: candidate records of one batch (tsg_ctx_options.cand_capacity); K2 drops the
// records past it and flags their files for whole-file resolution
int host_out_alloc(const DeviceRules* d, uint32_t files_cap, uint32_t cand_cap, HostOut* out);
void host_out_free(HostOut* o);

// The device part of one batch on lane `l`, asynchronously; out->ev[kEvDone] completes it.
int enqueue_scan(DeviceRules* d, LaneState* l, const ScanInput& in, HostOut* out);
// after out->ev[kEvDone]: the HIP-event times of that batch's stages
int batch_times(const HostOut* out, ScanTimes* t);
// keyword bits of the lane's last batch, as K1 / K1X left them on the device (test hook)
int lane_kw(LaneState* l, uint32_t* kw, size_t n);
// K1 output of the lane's last batch (test hook): chunk events [nchunks]
int lane_events(LaneState* l, uint32_t* ev, size_t n);
// K2's work lists of the lane's last batch as the item passes left them (test hook): list
// entries {group, first item, n, kind}, dense entries {group, first chunk, n, kind}, the
// item array (file, chunk) up to the layout's extent (or the array's end: the region of a
// skipped list group may lie past it), and the skip flags [groups]
struct LaneItems {
  std::vector<uint32_t> entries, dentries, items;
  std::vector<uint8_t> gskip;
  uint64_t extent = 0;  // the layout's extent (counter kCntItems)
};
int lane_items(LaneState* l, LaneItems* out);
// Every DevBuf member of the lane by name, with its capacity in bytes and the allocations it
// has had (test hook, tsg_test_lane_buffers): host values only, no device call.  A batch
// that found `allocs` as the previous batch on the lane left it ran in that batch's memory.
struct LaneBuffer {
  const char* name;
  uint64_t bytes, allocs;
};
void lane_buffers(const LaneState* l, std::vector<LaneBuffer>* out);
// K2 per-entry trace of the lane's last batch (TSG_K2_TRACE; empty otherwise): per entry
// {start, end, group << 32 | items, XCC_ID << 32 | HW_ID}
int lane_k2_trace(LaneState* l, std::vector<unsigned long long>* out);
int lane_k1f_trace(LaneState* l, std::vector<unsigned long long>* out);  // TSG_K1F_TRACE

// ---- device-resident input: the fetch of the files the host resolver reads
// The host lists the needed files as gather segments (adjacent files merged, each run cut to
// kGatherSegBytes so that one very large file spreads over many blocks).  A packed batch's
// have src == dst: fetch_kernel copies them from the caller's buffer into the batch's pinned
// slot at the same offsets.  A spans batch's go through gather_kernel, their source the
// files' spans.
constexpr uint64_t kGatherSegBytes = 64u << 10;
// The context's fetch stream (not a lane's: a lane may already run a later batch), its
// events and the pinned segment list.  Calls are serialized inside.
struct DeviceFetch;
int fetch_create(DeviceRules* d, DeviceFetch** out);
void fetch_destroy(DeviceFetch* f);
// host_dst[seg.dst, +len) = d_src[seg.dst, +len) for every listed segment (each with src ==
// dst) of the `total` bytes at d_src; host_dst is pinned, device-visible memory (a slot's
// data).  Synchronous; *ms = the kernel's HIP-event time.
int fetch_segments(DeviceFetch* f, const uint8_t* d_src, uint64_t total, uint8_t* host_dst,
                   const GatherSeg* segs, size_t nsegs, float* ms);
// Spans of a device buffer: flags[f] = utils.IsBinary of the span {starts[f], lengths[f]} of
// the base_bytes bytes at d_base (binary_gate_kernel on the fetch stream).  The three arrays
// are device addresses of pinned, host-mapped memory; the host has checked every span
// against the buffer.  Synchronous: the flags are readable on return; *ms = HIP-event time.
int gate_spans(DeviceFetch* f, const uint8_t* d_base, uint64_t base_bytes, const uint64_t* starts_dev,
               const uint64_t* lengths_dev, uint8_t* flags_dev, uint32_t nfiles, float* ms);
// host_dst[seg.dst, +len) = d_base[seg.src, +len) for every listed segment (gather_kernel);
// host_dst is pinned, device-visible memory of dst_bytes bytes.  Synchronous, as fetch_segments.
int fetch_gather(DeviceFetch* f, const uint8_t* d_base, uint64_t base_bytes, uint8_t* host_dst, uint64_t dst_bytes,
                 const GatherSeg* segs, size_t nsegs, float* ms);
// A layer tar in device memory: tar_mark_kernel's two bitmaps over the whole 512-byte blocks
// of the tar_len bytes at d_tar (any alignment), bit b % 64 of word b / 64 for block b.
// marks[0, words) = the block passes archive/tar's header checksum, marks[words, 2 * words) =
// the block is all zero, words = (tar_len / 512 + 63) / 64; both come back in one D2H.
// Synchronous; *ms = the kernel's HIP-event time.
int mark_tar(DeviceFetch* f, const uint8_t* d_tar, uint64_t tar_len, uint64_t* marks, float* ms);
// the whole batch in one runtime D2H (every file is needed)
int fetch_whole(DeviceFetch* f, const uint8_t* d_src, uint64_t total, uint8_t* host_dst, float* ms);

}  // namespace tsg
