// CPU emulation of the kernels' algorithm: the reference of the HIP kernels and of the CPU tests.
#include "plan.hpp"
#include "internal.hpp"

#include <algorithm>
#include <unordered_map>

namespace tsg {

void k1_reference(const Plan& plan, const BatchView& bv, uint32_t chunk, std::vector<uint32_t>* kw,
                  std::vector<uint32_t>* ev) {
  const uint32_t F = bv.nfiles;
  const uint64_t total = bv.offsets[F];
  const DFA& d = *plan.kw_dfa;
  const int nc = d.nclasses;
  const int W = plan.kw_words;
  kw->assign((size_t)F * W, 0);
  ev->assign((total + chunk - 1) / chunk, 0);
  uint32_t s = d.start[kCtxBOT];
  uint32_t cu = 0, cd = 0, f = 0;
  for (uint64_t p = 0; p < total; p++) {
    while (bv.offsets[f + 1] <= p) f++;  // the file holding byte p (skips empty files)
    const uint8_t c = bv.data[p];
    s = d.next[(size_t)s * nc + d.cls[c]];
    uint32_t e = 0;
    // arrival in state s: the literals its match set holds end with byte p
    const uint32_t mi = d.eot_acc[s];
    if (mi) {
      const auto& m = d.masks[mi];
      const uint64_t avail = p - bv.offsets[f] + 1;
      for (int k = 0; k < plan.n_kw; k++)
        if (((m[k / 64] >> (k % 64)) & 1) && plan.kw_len[k] <= avail)
          (*kw)[(size_t)f * W + k / 32] |= 1u << (k % 32);
      e |= plan.kw_mask_events[mi];
    }
    cu = (plan.run_cls[c] & 1) ? cu + 1 : 0;
    cd = (plan.run_cls[c] & 2) ? cd + 1 : 0;
    if ((int)cu >= plan.run_k[0]) e |= kEvRunU;
    if ((int)cd >= plan.run_k[1]) e |= kEvRunD;
    (*ev)[p / chunk] |= e;
  }
  k1x_reference(plan, bv, chunk, kw, ev);
}

// K1X semantics (the hashed literals of large rule sets): every occurrence of a literal in
// the ASCII-lowercased stream ending at byte q sets its event bits on chunk q / chunk, and
// its keyword bit for the file holding q when the whole literal lies inside that file.
void k1x_reference(const Plan& plan, const BatchView& bv, uint32_t chunk, std::vector<uint32_t>* kw,
                   std::vector<uint32_t>* ev) {
  if (plan.x_lits.empty()) return;
  const uint64_t total = bv.offsets[bv.nfiles];
  std::unordered_map<uint32_t, std::vector<uint32_t>> by4;
  for (size_t i = 0; i < plan.x_lits.size(); i++) by4[x_prefix4((const uint8_t*)plan.x_lits[i].data())].push_back((uint32_t)i);
  auto low = [](uint8_t c) -> uint8_t { return (c >= 'A' && c <= 'Z') ? (uint8_t)(c + 32) : c; };
  for (uint64_t p = 0; p + 4 <= total; p++) {
    const uint8_t b4[4] = {low(bv.data[p]), low(bv.data[p + 1]), low(bv.data[p + 2]), low(bv.data[p + 3])};
    auto it = by4.find(x_prefix4(b4));
    if (it == by4.end()) continue;
    for (uint32_t i : it->second) {
      const std::string& L = plan.x_lits[i];
      if (p + L.size() > total) continue;
      size_t t = 4;
      while (t < L.size() && low(bv.data[p + t]) == (uint8_t)L[t]) t++;
      if (t < L.size()) continue;
      const uint64_t q = p + L.size() - 1;
      (*ev)[q / chunk] |= plan.x_event[i];
      if (plan.x_kw[i] >= 0) {
        const uint32_t f = (uint32_t)(std::upper_bound(bv.offsets, bv.offsets + bv.nfiles + 1, q) - bv.offsets) - 1;
        if (p >= bv.offsets[f]) (*kw)[(size_t)f * plan.kw_words + plan.x_kw[i] / 32] |= 1u << (plan.x_kw[i] % 32);
      }
    }
  }
}

// K2's output form for one segment [a, b) of file [fs, fe) and the tail behind it (kernels.hip
// k2_list_pair, Lane::piece / streams, Lane::tail).  A word is 16 bytes of the batch, its part
// inside the segment or the tail.  In word form an accepting word becomes one kCandWord record
// {file, group, row before its first byte, that byte's offset}; in transition form every
// accepting transition becomes one kCandTrans record {file, group, row + class, its offset}.
// A tail stops at a word boundary past ext_cap or in an immortal state (kCandWhole for the
// group's rules); end-of-text accepts are per-rule candidates.  The list kernel at chunk sizes
// of whole 128-byte lines writes words for body and tail (TSG_EMU_WORDREC selects that form in
// emulate_kernels: it drives resolve_batch's word expansion without a device).
static void emulate_records(const DFA& d, uint32_t gi, const std::vector<uint32_t>& rules, const uint8_t* data,
                            uint32_t f, uint64_t fs, uint64_t fe, uint64_t a, uint64_t b, uint32_t ext_cap,
                            bool body_words, bool tail_words, std::vector<Candidate>* out) {
  const uint32_t nc = (uint32_t)d.nclasses, ncd = std::max<uint32_t>(2, nc);
  auto eot = [&](uint32_t s) {
    if (!d.eot_acc[s]) return;
    const auto& m = d.masks[d.eot_acc[s]];
    for (size_t k = 0; k < rules.size(); k++)
      if ((m[k / 64] >> (k % 64)) & 1) out->push_back({f, rules[k], (uint32_t)(fe - fs)});
  };
  // bytes [p, e) of one word from state s: the state after them, the word's records
  auto step = [&](uint32_t& s, uint64_t p, uint64_t e, bool words) {
    const uint32_t s0 = s;
    const uint64_t p0 = p;
    bool acc = false;
    for (; p < e; p++) {
      const uint32_t c = d.cls[data[p]];
      const size_t x = (size_t)s * nc + c;
      if (d.acc[x] && !words) out->push_back({f, kCandTrans | (gi << 16) | (s * ncd + c), (uint32_t)(p - fs)});
      acc |= d.acc[x] != 0;
      s = d.next[x];
    }
    if (acc && words) out->push_back({f, kCandTrans | kCandWord | (gi << 16) | (s0 * ncd), (uint32_t)(p0 - fs)});
  };
  uint32_t s = (a == fs) ? d.start[kCtxBOT] : d.start[DFA::ctx_of(data[a - 1], d)];
  for (uint64_t p = a; p < b;) {
    const uint64_t e = std::min<uint64_t>(b, (p | 15) + 1);
    step(s, p, e, body_words);
    p = e;
  }
  if (b >= fe) {
    eot(s);
    return;
  }
  s = d.to_noinject[s];
  uint64_t q = b;
  while (q < fe && !d.dead[s]) {
    if (q - b >= ext_cap || (s < d.immortal.size() && d.immortal[s])) {
      for (uint32_t r : rules) out->push_back({f, r, kCandWhole});
      return;
    }
    const uint64_t e = std::min<uint64_t>(fe, (q | 15) + 1);
    step(s, q, e, tail_words);
    q = e;
  }
  if (q >= fe && !d.dead[s]) eot(s);
}

void emulate_items(const Plan& plan, const BatchView& bv, uint32_t chunk, const uint32_t* kwbits,
                   const std::vector<uint32_t>& ev, uint32_t max_back,
                   const std::function<void(uint32_t g, uint32_t f, uint64_t c)>& visit) {
  const uint32_t F = bv.nfiles;
  for (size_t gi = 0; gi < plan.groups.size(); gi++) {
    const GroupPlan& g = plan.groups[gi];
    const uint32_t back = group_back(g, chunk);
    const bool every = (g.events & kEvAlways) != 0 || back > max_back;
    for (uint32_t f = 0; f < F; f++) {
      const uint64_t fs = bv.offsets[f], fe = bv.offsets[f + 1];
      if (fe == fs) continue;
      const uint32_t* kw = kwbits + (size_t)f * plan.kw_words;
      bool gate = g.always;
      for (int w = 0; w < plan.kw_words && !gate; w++) gate = (kw[w] & g.kwmask[w]) != 0;
      if (!gate) continue;
      const uint64_t c0 = fs / chunk, c1 = (fe - 1) / chunk;
      for (uint64_t c = c0; c <= c1; c++) {
        bool need = every;
        for (uint64_t q = c; q <= std::min<uint64_t>(c + back, c1) && !need; q++) need = (ev[q] & g.events) != 0;
        if (need) visit((uint32_t)gi, f, c);
      }
    }
  }
}

void layout_reference(const uint64_t* counts, uint32_t ngroups, uint64_t nchunks, uint64_t items_cap,
                      uint32_t max_dense, uint8_t* kind, LayoutTotals* totals) {
  LayoutTotals t;
  const uint64_t dense_all = (nchunks + kK2EntryChunks - 1) / kK2EntryChunks;
  uint64_t dense_wanted = 0;
  for (uint32_t g = 0; g < ngroups; g++) {
    const uint64_t cnt = counts[g];
    uint8_t k = kGroupNone;
    if (cnt * 2 > nchunks) {  // dense budget, in group order
      k = dense_wanted++ < max_dense ? kGroupDense : kGroupSkip;
      if (k == kGroupDense) t.dense_entries += dense_all;
    } else if (cnt) {  // then the item capacity; the region is kept either way
      k = t.extent + cnt <= items_cap ? kGroupList : kGroupSkip;
      if (k == kGroupList) t.entries += (cnt + kK2EntryItems - 1) / kK2EntryItems;
      t.extent += cnt;
    }
    t.skipped += k == kGroupSkip;
    if (kind) kind[g] = k;
  }
  if (totals) *totals = t;
}

void emulate_kernels(const Plan& plan, const BatchView& bv, uint32_t chunk, uint32_t ext_cap,
                     KernelOutput* ko, std::vector<uint64_t>* group_item_bytes, const EmuOptions* opt,
                     EmuStats* st) {
  const uint32_t F = bv.nfiles;
  const size_t G = plan.groups.size();
  const bool word_recs = knobs().emu_wordrec.load() && !knobs().k2_no_word_recs.load() && G <= 0x3FFF;
  const uint32_t max_back = opt ? opt->max_back : 0xFFFFFFFFu;
  std::vector<uint32_t> ev;
  k1_reference(plan, bv, chunk, &ko->kw, &ev);
  ko->cand.clear();
  ko->overflow.assign(F, 0);
  ko->group_skipped.clear();
  if (group_item_bytes) group_item_bytes->assign(G, 0);
  std::vector<uint8_t> kind;
  EmuStats es;
  if (opt && opt->layout) {
    std::vector<uint64_t> counts(G, 0);
    emulate_items(plan, bv, chunk, ko->kw.data(), ev, max_back, [&](uint32_t g, uint32_t, uint64_t) { counts[g]++; });
    kind.resize(G);
    layout_reference(counts.data(), (uint32_t)G, ev.size(), opt->items_cap, opt->max_dense, kind.data(), &es.layout);
    if (es.layout.skipped) {
      ko->group_skipped.assign(G, 0);
      for (size_t g = 0; g < G; g++) ko->group_skipped[g] = kind[g] == kGroupSkip;
    }
  }
  emulate_items(plan, bv, chunk, ko->kw.data(), ev, max_back, [&](uint32_t gi, uint32_t f, uint64_t c) {
    if (!kind.empty() && kind[gi] == kGroupSkip) return;  // left to the host (group_skipped)
    const GroupPlan& g = plan.groups[gi];
    const DFA& d = *g.dfa;
    const uint64_t fs = bv.offsets[f], fe = bv.offsets[f + 1];
    const uint64_t a = std::max<uint64_t>(fs, c * chunk), b = std::min<uint64_t>(fe, (c + 1) * chunk);
    if (group_item_bytes) (*group_item_bytes)[gi] += b - a;
    if (word_recs) {
      emulate_records(d, gi, g.rules, bv.data, f, fs, fe, a, b, ext_cap, true, true, &ko->cand);
      return;
    }
    bool o = run_segment(d, bv.data, fs, fe, a, b, ext_cap, [&](uint32_t mi, uint64_t pos) {
      const auto& m = d.masks[mi];
      for (size_t k = 0; k < g.rules.size(); k++)
        if ((m[k / 64] >> (k % 64)) & 1) ko->cand.push_back({f, g.rules[k], (uint32_t)pos});
    });
    if (o)  // a tail past ext_cap: the group's rules over the whole file (kCandWhole)
      for (uint32_t r : g.rules) ko->cand.push_back({f, r, kCandWhole});
  });
  es.candidates = ko->cand.size();
  // the candidate buffer's capacity, as emit_cand applies it: a record past it is dropped
  // and its file resolved whole
  if (opt && ko->cand.size() > opt->cand_cap) {
    for (size_t i = (size_t)opt->cand_cap; i < ko->cand.size(); i++) ko->overflow[ko->cand[i].file] = 1;
    ko->cand.resize((size_t)opt->cand_cap);
  }
  if (st) *st = es;
}

void emulate_candidates(const Plan& plan, const BatchView& bv, uint32_t chunk, uint32_t ext_cap, uint64_t items_cap,
                        uint32_t max_dense, bool word_recs, std::vector<Candidate>* out) {
  const uint32_t F = bv.nfiles;
  const size_t G = plan.groups.size();
  const uint64_t total = bv.offsets[F];
  const bool words = word_recs && G <= 0x3FFF;
  const bool fast_list = (chunk & 127) == 0;  // k2_list_pair's word loop; Lane::piece otherwise
  std::vector<uint32_t> kw, ev;
  k1_reference(plan, bv, chunk, &kw, &ev);
  std::vector<uint64_t> counts(G, 0);
  emulate_items(plan, bv, chunk, kw.data(), ev, kMaxBackChunks, [&](uint32_t g, uint32_t, uint64_t) { counts[g]++; });
  std::vector<uint8_t> kind(G, kGroupNone);
  layout_reference(counts.data(), (uint32_t)G, ev.size(), items_cap, max_dense, kind.data(), nullptr);
  out->clear();
  // list groups: one segment per item, the tail behind it capped at ext_cap
  emulate_items(plan, bv, chunk, kw.data(), ev, kMaxBackChunks, [&](uint32_t gi, uint32_t f, uint64_t c) {
    if (kind[gi] != kGroupList) return;
    const GroupPlan& g = plan.groups[gi];
    const uint64_t fs = bv.offsets[f], fe = bv.offsets[f + 1];
    const uint64_t a = std::max<uint64_t>(fs, c * chunk), b = std::min<uint64_t>(fe, (c + 1) * chunk);
    emulate_records(*g.dfa, gi, g.rules, bv.data, f, fs, fe, a, b, ext_cap, words && fast_list, words, out);
  });
  // dense groups (k2_dense_entry): every lane range of kStreams chunks; a range inside one
  // file is kStreams segments of a chunk each (Lane::streams), otherwise each file's part of
  // the range is one segment (Lane::piece); bodies in transition form
  constexpr uint64_t kStreams = 4;
  for (uint32_t gi = 0; gi < G; gi++) {
    if (kind[gi] != kGroupDense) continue;
    const GroupPlan& g = plan.groups[gi];
    auto gated = [&](uint32_t f) {
      if (g.always) return true;
      for (int w = 0; w < plan.kw_words; w++)
        if (kw[(size_t)f * plan.kw_words + w] & g.kwmask[w]) return true;
      return false;
    };
    auto segment = [&](uint32_t f, uint64_t a, uint64_t b) {
      emulate_records(*g.dfa, gi, g.rules, bv.data, f, bv.offsets[f], bv.offsets[f + 1], a, b, ext_cap, false, words, out);
    };
    uint32_t f = 0;
    for (uint64_t a = 0; a < total; a += kStreams * chunk) {
      const uint64_t b = std::min<uint64_t>(a + kStreams * chunk, total);
      while (bv.offsets[f + 1] <= a) f++;  // the file of byte a
      if (b == a + kStreams * chunk && b <= bv.offsets[f + 1]) {
        if (gated(f))
          for (uint64_t i = 0; i < kStreams; i++) segment(f, a + i * chunk, a + (i + 1) * chunk);
        continue;
      }
      uint32_t h = f;
      for (uint64_t p = a; p < b; h++) {
        const uint64_t fe = bv.offsets[h + 1];
        if (fe <= p) continue;
        const uint64_t se = std::min(b, fe);
        if (gated(h)) segment(h, p, se);
        p = se;
      }
    }
  }
}
}  // namespace tsg
