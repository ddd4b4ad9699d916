// Compiled plan for the GPU pipeline of one rule set, and the host resolver.
//
//   K1  keyword automaton  : every distinct lowercased ASCII keyword of every rule
//                            (Rule.MatchKeywords, scanner.go:164-176) + two pseudo
//                            keywords for the only non-ASCII runes whose simple
//                            lowercase is ASCII (U+0130 -> 'i', U+212A -> 'k'); a file
//                            containing them gets its keyword gate checked exactly.
//   K2  rule-group DFAs    : the rules' regexes packed into groups (one DFA each,
//                            accept bit per rule); a group is scanned only over the
//                            files whose keyword bits gate at least one of its rules.
//   resolver (host)        : candidate end offsets -> exact windows -> scan_file.
#pragma once
#include <cstdint>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "dfa.hpp"
#include "scanner.hpp"

namespace tsg {

enum KwMode : uint8_t { kKwAlways = 0, kKwBits = 1, kKwUnknown = 2 };

// Chunk events (K1 output, one u32 per chunk of the batch).  A rule group is scanned by
// K2 only over the chunks of its gated files that lie within `back` chunks before a
// chunk carrying one of its event bits (see Plan::rule_event).
constexpr uint32_t kEvRunU = 1u;        // run of >= run_k[0] bytes of class U
constexpr uint32_t kEvRunD = 2u;        // run of >= run_k[1] bytes of class D
constexpr int kEvLit0 = 2;              // bits 2..30: anchor literal classes
constexpr int kEvLitBits = 29;
constexpr uint32_t kEvAlways = 1u << 31;  // implicit in every chunk

struct GroupPlan {
  std::unique_ptr<DFA> dfa;
  std::vector<uint32_t> rules;   // group-local accept id -> global rule index
  std::vector<uint32_t> kwmask;  // keyword ids gating this group [kw_words]
  bool always = false;           // some member rule is not keyword-gated on the GPU
  uint32_t events = kEvAlways;   // OR of the member rules' event bits
  int64_t evdist = 0;            // max over members of Plan::rule_evdist
};

struct Plan {
  // K1: Aho-Corasick automaton over literal ids [0, n_kw) keywords (incl. the 3 fallback
  // pseudo keywords at fb_kw0..), [n_kw, n_lit) anchor literals that are not keywords.
  // Its accepts are state-based; kw_mask_events[m] = event bits of accept mask m.
  std::unique_ptr<DFA> kw_dfa;
  int n_kw = 0;        // keyword ids incl. the 3 fallback pseudo keywords at the end
  int n_lit = 0;
  int kw_words = 1;    // 32-bit words per file
  int fb_kw0 = 0;      // first fallback pseudo keyword id
  std::vector<uint32_t> kw_mask_events;
  std::vector<uint32_t> lit_event;     // [n_lit] event bits of each literal
  std::vector<std::string> k1_lits;    // [n_lit] the automaton's literals (ASCII case folded
                                       // when matched); a keyword left out is
                                       // never_literal() (dfa.hpp: matches nothing)
  std::vector<uint16_t> kw_len;        // [n_kw] byte length of each keyword literal
  // K1X: literals of >= 4 bytes that K1's LDS-resident automaton has no room for (large
  // user rule sets) -- keywords, and anchor literals with their event bits -- found by a
  // hashed 4-gram prefilter and exact verification (k1x_kernel).  Same semantics as
  // K1's: ASCII case folded, one stream, a keyword counts only inside one file.
  std::vector<std::string> x_lits;     // ASCII-lowercased literal bytes
  std::vector<int32_t> x_kw;           // keyword id, or -1 (anchor only)
  std::vector<uint32_t> x_event;       // event bits (0: keyword only)
  int x_step = 1;                      // K1X samples a 4-byte window every x_step bytes
  std::vector<uint8_t> x_j0;           // K1X windows of literal i: offsets x_j0[i] .. + x_step - 1
  // run classes for kEvRunU / kEvRunD: byte -> membership bit 0 (U) / 1 (D)
  uint8_t run_cls[256] = {0};
  int run_k[2] = {32, 12};
  int warm = 32;       // K1 warm-up bytes before a chunk (>= longest literal - 1, >= run_k - 1)
  // per rule: event bits (kEvAlways = none) and the largest distance in bytes from the
  // start of a match of the rule's GPU program to the event byte inside it; the
  // program keeps atoms [rule_first_atom, ...) of the regex
  std::vector<uint32_t> rule_event;
  std::vector<int64_t> rule_evdist;
  std::vector<int> rule_first_atom;
  std::vector<std::string> rule_anchor;  // description, for plan reports
  std::vector<uint8_t> rule_kw_mode;            // per rule
  std::vector<std::vector<uint32_t>> rule_kws;  // per rule: keyword ids
  std::vector<GroupPlan> groups;
  std::vector<int> rule_group;       // per rule: group index, -1 = no GPU DFA
  std::vector<uint8_t> rule_hostonly;  // regex without a GPU DFA (host scans gated files)
  std::vector<int64_t> rule_maxlen;  // longest EXACT match in bytes, -1 unbounded
  std::vector<int> rule_relax;       // relaxation used for the GPU program (-1 exact)
  std::vector<int> rule_atoms;       // GPU program = prefix of this many atoms (-1 = all)
  // a GPU end offset e says "a match may START in [e - winback, e]" (-1: anywhere before e)
  std::vector<int64_t> rule_winback;
  std::vector<Prog> rule_prog;       // the program the rule's GPU DFA was built from
  // reverse DFA of the exact program (null: state cap): bounds and filters the windows
  std::vector<std::unique_ptr<DFA>> rule_rev;
  // unbounded rules with a relaxed GPU program: a relaxed forward DFA that also accepts
  // U+017F / U+212A where (?i) folds s / k (null: state cap or not needed).  Run on the
  // host over a file holding those runes, it gives candidate ends instead of a whole-file
  // FindAll.
  std::vector<std::unique_ptr<DFA>> rule_fold_dfa;
  // The unbounded rules' fold programs (rule_fold_dfa's, or the GPU program of an unrelaxed
  // rule, which keeps U+017F / U+212A) in ONE forward DFA, accept id k = fold_rules[k]: one
  // pass over a file with folding runes gives every such rule's candidate ends (null: state
  // cap; the per-rule DFAs are used)
  std::unique_ptr<DFA> fold_all_dfa;
  std::vector<uint32_t> fold_rules;
  std::unique_ptr<DFA> allow_path_dfa;  // Global.AllowPath on ASCII paths
};

struct PlanOptions {
  int max_group_states = 1024;
  int max_group_table_bytes = 48 * 1024;
  int max_rules_per_group = 64;
  int max_kw_table_bytes = 96 * 1024;  // K1 transition table must stay LDS-resident
};

std::unique_ptr<Plan> build_plan(const Ruleset& rs, const PlanOptions& opt, std::string* err);

// 64-bit FNV-1a hash of a canonical serialisation of every member of the plan (test hook
// tsg_ruleset_plan_digest): equal digests, equal plans.
uint64_t plan_digest(const Plan& p);

// One GPU candidate: rule `rule` has a match ending at byte `end` of file `file`, or, with
// end == kCandWhole, the rule's K2 thread ran past ext_cap: resolve the rule over the whole
// file (only that rule: the other rules of the file keep their windows).
constexpr uint32_t kCandWhole = 0xFFFFFFFFu;
// Candidate.rule with this bit: a K2 transition record {group g = bits 16-30, table index ix
// = bits 0-15 (state * max(2, nclasses) + class of the group's DFA)}: the transition at
// `end` accepts, and its accept mask names the rules (expanded on the host, so the kernel
// looks up no mask per accepting byte)
constexpr uint32_t kCandTrans = 0x80000000u;
// with kCandTrans: a whole accepting 16-B word {file, kCandTrans | kCandWord | group << 16 |
// row before the byte at end, end}; the host replays it (groups then have 14 bits)
constexpr uint32_t kCandWord = 0x40000000u;
struct Candidate {
  uint32_t file;
  uint32_t rule;
  uint32_t end;
};

// What the kernels hand back for one batch, wherever it lives (pinned host buffers of the
// device pipeline, or the vectors of a CPU emulation).
struct KernelOutputView {
  const uint32_t* kw = nullptr;     // [nfiles * kw_words]
  const Candidate* cand = nullptr;
  size_t ncand = 0;
  const uint8_t* overflow = nullptr;    // [nfiles] or null: bit 0 = resolve the whole file exactly
  // overflow bit 1 = folding runes present (their keyword bits set), bit 2 = the file's
  // keyword row is written, and `kw` holds only those rows (files with candidates or a flag
  // set: the device's outputs kernel); otherwise `kw` is whole and folding runes are read
  // from it
  bool sparse_kw = false;
  const uint8_t* kw_unknown = nullptr;  // [n_kw] or null: keyword bits K1 no longer reports
  const uint8_t* path_ok = nullptr;     // [nfiles] or null: Global.AllowPath from the device
  // [groups] or null: groups K2 did not scan in this batch (item capacity); their rules are
  // resolved like rules without a GPU program
  const uint8_t* group_skipped = nullptr;
};

// How K2 covers a rule group in one batch (kernels.hip layout_block, layout_reference).
enum : uint8_t { kGroupNone = 0, kGroupList = 1, kGroupDense = 2, kGroupSkip = 3 };
// The device's item rules: a group whose event window is longer than kMaxBackChunks chunks
// listens to every chunk of its gated files; a list entry holds up to kK2EntryItems items
// of one group, a dense entry kK2EntryChunks consecutive chunks of the batch.
constexpr uint32_t kMaxBackChunks = 16;
constexpr uint32_t kK2EntryItems = 512;
constexpr uint32_t kK2EntryChunks = 1024;

// layout_block's decision restated on the host, groups in id order: a group whose items
// cover more than half of the batch's chunks wants the dense pass and gets it while fewer
// than max_dense groups before it wanted it; every other group with items wants a region of
// the item array at the sum of the list-wanting counts before it (a skipped group keeps its
// region) and is listed when that region ends within items_cap.  A group with items that
// gets neither is skipped.
struct LayoutTotals {
  uint64_t extent = 0;         // item array in use: regions of every list-wanting group
  uint64_t entries = 0;        // list entries
  uint64_t dense_entries = 0;  // dense entries
  uint64_t skipped = 0;        // skipped groups
};
void layout_reference(const uint64_t* counts, uint32_t ngroups, uint64_t nchunks, uint64_t items_cap,
                      uint32_t max_dense, uint8_t* kind, LayoutTotals* totals);

// Everything the kernels hand back for one batch.
struct KernelOutput {
  std::vector<uint32_t> kw;        // [nfiles * kw_words]
  std::vector<Candidate> cand;
  std::vector<uint8_t> overflow;   // [nfiles] 1 = resolve the whole file exactly
  // [n_kw] (or empty): keyword bits K1 no longer reports (a clear bit proves nothing)
  std::vector<uint8_t> kw_unknown;
  // [nfiles] (or empty): Global.AllowPath of each path computed on the device:
  // 0 / 1, or 2 = non-ASCII path, decided on the host
  std::vector<uint8_t> path_ok;
  // [groups] (or empty): 1 = the layout skipped the group, it has no candidates
  std::vector<uint8_t> group_skipped;
  KernelOutputView view() const {
    KernelOutputView v;
    v.kw = kw.data();
    v.cand = cand.data();
    v.ncand = cand.size();
    v.overflow = overflow.empty() ? nullptr : overflow.data();
    v.kw_unknown = kw_unknown.empty() ? nullptr : kw_unknown.data();
    v.path_ok = path_ok.empty() ? nullptr : path_ok.data();
    v.group_skipped = group_skipped.empty() ? nullptr : group_skipped.data();
    return v;
  }
};

struct BatchView {
  const uint8_t* data;
  const uint64_t* offsets;  // [nfiles + 1]
  uint32_t nfiles;
  const char* paths;
  const uint64_t* path_offsets;  // [nfiles + 1]
};

// The rules the host resolves alone in this batch: those without a GPU program and those of
// a group K2 skipped.  While there is one, every file needs the exact scan.
std::vector<uint32_t> host_rules(const Plan& plan, const KernelOutputView& ko);

// Does the host resolver read file f's bytes (resolve_batch), or is the file settled by
// Global.AllowPath alone?  It reads a file with a candidate record, an empty file, a file
// whose overflow flag (bit 0) is set, a file with folding-rune keyword bits, and every file
// while a host rule exists (any_host: !host_rules().empty()).  The one predicate of the
// resolver and of the fetch of a device-resident batch (pipeline.cpp), whose pinned mirror
// holds only the files this names: has_cand is "a candidate of f after the expansion of word
// records" in the resolver and "a record of f" in the fetch, which includes it.
inline bool file_needs_scan(const Plan& plan, const KernelOutputView& ko, uint32_t f, bool has_cand, bool empty,
                            bool any_host) {
  if (has_cand || empty || (ko.overflow && (ko.overflow[f] & 1)) || any_host) return true;
  if (ko.sparse_kw) return (ko.overflow[f] & 2) != 0;
  const uint32_t* kw = ko.kw + (size_t)f * plan.kw_words;
  for (int k = plan.fb_kw0; k < plan.n_kw; k++)
    if ((kw[k / 32] >> (k % 32)) & 1) return true;
  return false;
}

// Start offsets of the folding runes in s: which = 1 U+0130, 2 U+212A, 4 U+017F (ORed).
void fold_rune_positions(const uint8_t* s, int64_t n, uint32_t which, std::vector<int64_t>* out);

// Host resolution: exact findings for every file of the batch.
void resolve_batch(const Ruleset& rs, const Plan& plan, const BatchView& b,
                   const KernelOutputView& ko, int nthreads, BatchResult* out);

// Exact CPU path for a whole batch (no GPU).
void scan_batch_cpu(const Ruleset& rs, const BatchView& b, int nthreads,
                    std::vector<FileResult>* out);

// CPU emulation of the two kernels' algorithm (same chunking, same tables);
// used by the CPU tests and as the reference for the HIP kernels.
// group_item_bytes (optional, [groups]): bytes of the K2 items of each group.
// opt (optional): the device's rules on top of the algorithm, as an emulated context
// applies them; st (optional): what the device would count.
struct EmuOptions {
  uint32_t max_back = 0xFFFFFFFFu;  // emulate_items' max_back (the device: kMaxBackChunks)
  bool layout = false;              // layout_reference decides: a skipped group has no candidates
  uint64_t items_cap = 0;
  uint32_t max_dense = 0;
  uint64_t cand_cap = ~0ull;  // records past it are dropped and their files flagged (overflow)
};
struct EmuStats {
  uint64_t candidates = 0;  // records produced, dropped ones included
  LayoutTotals layout;
};
void emulate_kernels(const Plan& plan, const BatchView& b, uint32_t chunk, uint32_t ext_cap,
                     KernelOutput* ko, std::vector<uint64_t>* group_item_bytes = nullptr,
                     const EmuOptions* opt = nullptr, EmuStats* st = nullptr);

// What K2 writes for one batch, record by record, in the device's own form and under the
// device's rules (tests: compared with the records read back from the device).  Items come
// from emulate_items(max_back = kMaxBackChunks) and the kinds from layout_reference; a
// skipped group has no records.
//   list group, chunk a multiple of 128 (k2_list_pair's word loop): per item, one kCandWord
//     record per accepting 16-B word of the body and of the tail
//   list group, other chunk sizes (Lane::piece): the body writes one kCandTrans record per
//     accepting transition, the tail word records
//   dense group (k2_dense_entry): every lane range of 4 consecutive chunks of the batch; a
//     range that lies in one gated file is four segments of a chunk, each with its own tail
//     (Lane::streams), otherwise each gated file's part of the range is one segment with one
//     tail (Lane::piece); bodies write transition records, tails word records
//   word_recs = false (the k2_no_word_recs knob; always with 16,384 groups and more): every
//     word record above is the word's transition records instead (Lane::replay_emit)
// Everywhere: end-of-text accepts are per-rule candidates {file, rule, file length}, and a
// tail alive at a word boundary >= ext_cap bytes behind its segment, or in an immortal state,
// ends with {file, rule, kCandWhole} for every rule of the group.  No capacity is applied.
void emulate_candidates(const Plan& plan, const BatchView& b, uint32_t chunk, uint32_t ext_cap, uint64_t items_cap,
                        uint32_t max_dense, bool word_recs, std::vector<Candidate>* out);

// The candidates of one K2 record appended to out: a plain candidate (kCandWhole included)
// as it is, a transition record as one candidate per rule of its accept mask, a word record
// as the candidates of every accepting transition from its byte to the end of its 16-B word
// of the batch (or of the file).  A record that names no group, state or file of the plan
// and batch gives nothing.
void expand_candidate(const Plan& plan, const BatchView& b, const Candidate& c, std::vector<Candidate>* out);

// The item set K2 scans, given K1's output (kw [nfiles * kw_words], ev [chunks]): visit(g, f,
// c) for every group g, file f and chunk c, in that order, such that g is gated for f
// (always, or kw & kwmask), c is a chunk of f, and some chunk in [c, min(c + back_g, last
// chunk of f)] carries one of g's event bits.  Empty files have no items.  A group with
// back_g > max_back listens to every chunk (the device: kMaxBackChunks; 0xFFFFFFFF: never).
void emulate_items(const Plan& plan, const BatchView& b, uint32_t chunk, const uint32_t* kw,
                   const std::vector<uint32_t>& ev, uint32_t max_back,
                   const std::function<void(uint32_t g, uint32_t f, uint64_t c)>& visit);

// K1 semantics shared by the HIP kernel and the emulation: keyword bits of every file
// [nfiles * kw_words] and event bits of every chunk c = bytes [c*chunk, (c+1)*chunk).
// The automaton and the run counters run over the batch as ONE byte stream (they are not
// reset at file boundaries), so a chunk's event bits are a superset of its files' own.
// Keyword bits stay exact: an occurrence counts for file f only when the whole keyword
// lies inside f (its length is checked against the bytes of f before its last byte).
void k1_reference(const Plan& plan, const BatchView& b, uint32_t chunk,
                  std::vector<uint32_t>* kw, std::vector<uint32_t>* ev);
// The K1X part of k1_reference (Plan::x_lits), ORed into kw / ev.
void k1x_reference(const Plan& plan, const BatchView& b, uint32_t chunk,
                   std::vector<uint32_t>* kw, std::vector<uint32_t>* ev);

// K1X: the 4-byte little-endian prefix word of a (lowercased) literal or window
inline uint32_t x_prefix4(const uint8_t* b) {
  return (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
}
// K1X prefilter: a blocked Bloom filter of 2^kXDwordBits dwords (128 KiB of LDS).  A
// window's hash picks one dword and two bits in it; the window passes when both are set.
constexpr int kXDwordBits = 15;
constexpr uint32_t kXDwords = 1u << kXDwordBits;
// Keys are folded windows: bit 5 of every byte set, so an ASCII letter and its capital agree
// (one OR per dword on the device instead of a lowercase).
constexpr uint32_t kXFold = 0x20202020u;
inline uint32_t x_fold(uint32_t w) { return w | kXFold; }
inline uint32_t x_hash(uint32_t w) { return w * 2654435761u; }
inline uint32_t x_dword(uint32_t h) { return h >> (32 - kXDwordBits); }
inline uint32_t x_bits(uint32_t h) { return 1u << ((h >> 12) & 31) | 1u << ((h >> 7) & 31); }

// Chunks of file f that K2 scans for group g (given the K1 output): chunk c of the file
// is an item iff the group is gated for f and a chunk in [c, c + back] (inside f)
// carries one of the group's event bits.  back = ceil(evdist / chunk).
inline uint32_t group_back(const GroupPlan& g, uint32_t chunk) {
  return (uint32_t)((g.evdist + chunk - 1) / chunk);
}

}  // namespace tsg
