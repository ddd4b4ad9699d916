// Host resolver: K2's candidate records -> exact windows -> scan_file; the exact CPU batch path.
#include "plan.hpp"
#include "internal.hpp"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <stdexcept>
#include <x86intrin.h>

namespace tsg {

bool path_allowed(const Ruleset& rs, const Plan* plan, const char* p, size_t n) {
  if (plan && plan->allow_path_dfa) {
    bool ascii = true;
    for (size_t i = 0; i < n && ascii; i++) ascii = (uint8_t)p[i] < 0x80;
    if (ascii) {  // any accept (a non-empty mask) = some allow path regexp matches
      const DFA& d = *plan->allow_path_dfa;
      uint32_t s = d.start[kCtxBOT];
      for (size_t i = 0; i < n; i++) {
        const size_t e = (size_t)s * d.nclasses + d.cls[(uint8_t)p[i]];
        if (d.acc[e]) return true;
        s = d.next[e];
      }
      return d.eot_acc[s] != 0;
    }
  }
  return rs.AllowPath(std::string(p, n));
}

void scan_batch_cpu(const Ruleset& rs, const BatchView& b, int nthreads,
                    std::vector<FileResult>* out) {
  out->assign(b.nfiles, FileResult{});
  pool_for(b.nfiles, nthreads, [&](size_t i) {
    std::string path(b.paths + b.path_offsets[i], b.path_offsets[i + 1] - b.path_offsets[i]);
    scan_file(rs, path, b.data + b.offsets[i], b.offsets[i + 1] - b.offsets[i], nullptr,
              &(*out)[i]);
  });
}

// rune boundary at or before p in the canonical (from-0) UTF-8 segmentation
static int64_t align_rune(const uint8_t* d, int64_t n, int64_t p) {
  if (p <= 0) return 0;
  if (p >= n) return n;
  if ((d[p] & 0xC0) != 0x80) return p;
  for (int k = 1; k <= 3 && p - k >= 0; k++) {
    int64_t q = p - k;
    if ((d[q] & 0xC0) != 0x80) {
      int w;
      decode_rune(d, (size_t)n, (size_t)q, &w);
      return (q + w > p) ? q : p;
    }
  }
  return p;
}
std::vector<uint32_t> host_rules(const Plan& plan, const KernelOutputView& ko) {
  std::vector<uint32_t> out;
  for (size_t r = 0; r < plan.rule_hostonly.size(); r++)
    if (plan.rule_hostonly[r] ||
        (ko.group_skipped && plan.rule_group[r] >= 0 && ko.group_skipped[plan.rule_group[r]]))
      out.push_back((uint32_t)r);
  return out;
}

// one record's candidates into `out` (a word record replays its word from the batch)
void expand_candidate(const Plan& plan, const BatchView& b, const Candidate& c, std::vector<Candidate>* out) {
  if (!(c.rule & kCandTrans) || c.end == kCandWhole) {
    out->push_back(c);
    return;
  }
  const bool words = plan.groups.size() <= 0x3FFF;  // kCandWord records (kernels.hip accept_word)
  const bool word = words && (c.rule & kCandWord);
  const uint32_t g = (c.rule >> 16) & (words ? 0x3FFFu : 0x7FFFu), ix = c.rule & 0xFFFFu;
  if (g >= plan.groups.size()) return;
  const GroupPlan& gp = plan.groups[g];
  const DFA& d = *gp.dfa;
  const uint32_t ncd = (uint32_t)std::max(2, d.nclasses);  // the device's row width
  if (word) {  // kCandWord: replay the word from row ix at byte `end` to the word's end
    size_t st = ix / ncd;
    if (st >= (size_t)d.nstates || c.file >= b.nfiles) return;
    const uint64_t f0 = b.offsets[c.file], flen = b.offsets[c.file + 1] - f0;
    const uint64_t pend = std::min<uint64_t>(flen, (((f0 + c.end) | 15) + 1) - f0);
    for (uint64_t p = c.end; p < pend; p++) {
      const size_t e = st * d.nclasses + d.cls[b.data[f0 + p]];
      if (d.acc[e]) {
        const auto& m = d.masks[d.acc[e]];
        for (size_t k = 0; k < gp.rules.size(); k++)
          if ((m[k / 64] >> (k % 64)) & 1) out->push_back({c.file, gp.rules[k], (uint32_t)p});
      }
      st = d.next[e];
    }
    return;
  }
  const size_t st = ix / ncd, cl = std::min<size_t>(ix % ncd, (size_t)d.nclasses - 1);
  if (st >= (size_t)d.nstates) return;
  const auto& m = d.masks[d.acc[st * d.nclasses + cl]];
  for (size_t k = 0; k < gp.rules.size(); k++)
    if ((m[k / 64] >> (k % 64)) & 1) out->push_back({c.file, gp.rules[k], c.end});
}

void resolve_batch(const Ruleset& rs, const Plan& plan, const BatchView& b,
                   const KernelOutputView& ko, int nthreads, BatchResult* out) {
  const uint32_t F = b.nfiles;
  const size_t R = rs.rules.size();
  const uint64_t t_ser0 = __rdtsc();
  // K2 transition records (kCandTrans) -> one candidate per rule of their accept mask
  std::vector<Candidate> expanded;
  const Candidate* kc = ko.cand;
  size_t nkc = ko.ncand;
  {
    size_t ntrans = 0;
    for (size_t i = 0; i < nkc; i++) ntrans += (kc[i].rule & kCandTrans) && kc[i].end != kCandWhole;
    if (ntrans) {
      // In parallel, in record order: each word record's replay reads the batch at its own
      // place (a cache and TLB miss in a pinned multi-GiB slot), and serially that was half
      // of a layer piece's resolution (12-15 of ~28 Mcyc per 256 MiB piece, TSG_PROF).
      constexpr size_t kRecBlk = 2048;
      const size_t nrb = (nkc + kRecBlk - 1) / kRecBlk;
      std::vector<std::vector<Candidate>> parts(nrb);
      pool_for(nrb, nthreads, [&](size_t bi) {
        auto& out = parts[bi];
        const size_t i1 = std::min(nkc, (bi + 1) * kRecBlk);
        out.reserve(i1 - bi * kRecBlk + 16);
        for (size_t i = bi * kRecBlk; i < i1; i++) expand_candidate(plan, b, kc[i], &out);
      }, 1);
      size_t total = 0;
      for (const auto& pt : parts) total += pt.size();
      expanded.reserve(total);
      for (const auto& pt : parts) expanded.insert(expanded.end(), pt.begin(), pt.end());
      kc = expanded.data();
      nkc = expanded.size();
    }
  }
  // bucket candidates by file (counting sort), then sort each file's few by (rule, end)
  std::vector<uint32_t> first(F + 1, 0);
  for (size_t i = 0; i < nkc; i++) first[kc[i].file + 1]++;
  for (uint32_t f = 0; f < F; f++) first[f + 1] += first[f];
  std::vector<Candidate> cand(nkc);
  {
    std::vector<uint32_t> fill(first.begin(), first.end() - 1);
    for (size_t i = 0; i < nkc; i++) cand[fill[kc[i].file]++] = kc[i];
  }
  auto by_rule_end = [](const Candidate& x, const Candidate& y) {
    return x.rule != y.rule ? x.rule < y.rule : x.end < y.end;
  };

  const std::vector<uint32_t> hostonly = host_rules(plan, ko);
  std::vector<uint8_t> kw_has_i(R, 0), kw_has_k(R, 0);
  for (size_t r = 0; r < R; r++)
    for (const auto& k : rs.rules[r].kw_lower) {
      kw_has_i[r] |= k.find('i') != std::string::npos;
      kw_has_k[r] |= k.find('k') != std::string::npos;
    }

  const uint64_t t_ser1 = __rdtsc();
  // Global.AllowPath (scanner.go:343-347): from the device when it decided the path
  auto path_ok = [&](uint32_t f) -> bool {
    if (ko.path_ok && ko.path_ok[f] < 2) return ko.path_ok[f] == 1;
    return path_allowed(rs, &plan, b.paths + b.path_offsets[f], b.path_offsets[f + 1] - b.path_offsets[f]);
  };
  // Files that need the exact scan: candidates, empty files, kernel overflow, folding
  // runes, or a gated rule without a GPU program.  The others only need Global.AllowPath,
  // settled here.  Two parallel passes over blocks of files: flags and counts, then slot
  // numbers in file order.
  out->status.resize(F);
  out->slot.resize(F);
  const size_t kBlk = 8192, nblk = (F + kBlk - 1) / kBlk;
  std::vector<uint32_t> bcount(nblk + 1, 0);
  pool_for(nblk, nthreads, [&](size_t bi) {
    uint32_t cnt = 0;
    for (uint32_t f = (uint32_t)(bi * kBlk), fe = (uint32_t)std::min<size_t>(F, (bi + 1) * kBlk); f < fe; f++) {
      if (file_needs_scan(plan, ko, f, first[f] != first[f + 1], b.offsets[f + 1] == b.offsets[f], !hostonly.empty())) {
        out->slot[f] = 0;
        cnt++;
      } else {
        out->slot[f] = UINT32_MAX;
        out->status[f] = path_ok(f) ? kPathAllowed : kNoFindings;
      }
    }
    bcount[bi + 1] = cnt;
  }, 1);
  for (size_t bi = 0; bi < nblk; bi++) bcount[bi + 1] += bcount[bi];
  const uint32_t nslots = bcount[nblk];
  std::vector<uint32_t> need_files(nslots);
  pool_for(nblk, nthreads, [&](size_t bi) {
    uint32_t k = bcount[bi];
    for (uint32_t f = (uint32_t)(bi * kBlk), fe = (uint32_t)std::min<size_t>(F, (bi + 1) * kBlk); f < fe; f++)
      if (out->slot[f] != UINT32_MAX) {
        out->slot[f] = k;
        need_files[k++] = f;
      }
  }, 1);
  out->res.clear();
  out->res.resize(nslots);
  // a sparse keyword array holds only the rows the device wrote (flag bit 2): every file
  // that needs resolution must have one (reading any other row would read stale bits).
  // Checked here on the caller, not inside the parallel pass: a throw from a pool worker
  // would terminate the process.
  if (ko.sparse_kw)
    for (uint32_t f : need_files)
      if (b.offsets[f + 1] != b.offsets[f] && !(ko.overflow[f] & 4))
        throw std::runtime_error("keyword row of a resolved file not written");

  static const bool prof = getenv("TSG_PROF") != nullptr;
  if (prof)
    fprintf(stderr, "resolve: setup %.1f Mcyc (candidate sort %.1f; %u files to scan)\n", (__rdtsc() - t_ser0) / 1e6,
            (t_ser1 - t_ser0) / 1e6, nslots);
  // TSG_PROF: per-thread cycle counters (no shared atomics in the loop)
  struct alignas(64) Slot {
    // fast files, candidate files, other files, count cand, scan_file, fold-rune keyword
    // windows, fold windows of bounded rules, fold DFA / group DFA whole-file runs
    uint64_t cyc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  };
  static std::atomic<int> next_tid{0};
  std::vector<Slot> slots(prof ? 256 : 0);
  std::atomic<int64_t> n_whole{0};
  const uint64_t t_par0 = prof ? __rdtsc() : 0;
  pool_for(nslots, nthreads, [&](size_t si) {
    thread_local int tid = next_tid++ & 255;
    const uint64_t tp0 = prof ? __rdtsc() : 0;
    struct Tm {
      bool on;
      uint64_t t0;
      uint64_t* acc;
      ~Tm() {
        if (on) *acc += __rdtsc() - t0;
      }
    };
    const uint32_t f = need_files[si];
    const bool has_cand = first[f] != first[f + 1];
    Tm tm{prof, tp0, prof ? &slots[tid].cyc[has_cand ? 1 : 2] : nullptr};
    if (prof && has_cand) slots[tid].cyc[3]++;
    const char* pp = b.paths + b.path_offsets[f];
    const size_t pn = b.path_offsets[f + 1] - b.path_offsets[f];
    const uint8_t* content = b.data + b.offsets[f];
    const int64_t n = (int64_t)(b.offsets[f + 1] - b.offsets[f]);
    FileResult& res = out->res[out->slot[f]];
    struct SetStatus {
      FileResult& r;
      uint8_t& s;
      ~SetStatus() { s = r.status; }
    } set_status{res, out->status[f]};
    if (n == 0) {  // the kernels skip empty files; only empty matches are possible
      scan_file(rs, std::string(pp, pn), content, 0, nullptr, &res);
      return;
    }
    // (a sparse keyword array has this file's row: checked before the parallel pass)
    const uint32_t* kw = ko.kw + (size_t)f * plan.kw_words;
    // folding runes present: bit 0 U+0130, bit 1 U+212A, bit 2 U+017F
    uint32_t fbbits = 0;
    for (int k = plan.fb_kw0; k < plan.n_kw; k++)
      if ((kw[k / 32] >> (k % 32)) & 1) fbbits |= 1u << (k - plan.fb_kw0);
    // Keyword gate.  K1 bits are exact for the ASCII bytes of the file; bytes.ToLower
    // turns a non-ASCII rune into an ASCII letter only for U+0130 -> 'i' and U+212A -> 'k',
    // so a clear bit is uncertain only for keywords holding that letter.
    auto kw_state = [&](size_t r) -> uint8_t {
      switch (plan.rule_kw_mode[r]) {
        case kKwAlways: return 1;
        case kKwUnknown: return 2;
        default:
          for (uint32_t k : plan.rule_kws[r])
            if ((kw[k / 32] >> (k % 32)) & 1) return 1;
          if (ko.kw_unknown)
            for (uint32_t k : plan.rule_kws[r])
              if (ko.kw_unknown[k]) return 2;  // the kernels scanned the rule's group
          // 3: uncertain and the kernels did not scan the rule (its keyword bits were clear)
          if (((fbbits & 1) && kw_has_i[r]) || ((fbbits & 2) && kw_has_k[r])) return 3;
          return 0;
      }
    };
    // kernel overflow: resolve every rule over the whole file
    const bool ovf = ko.overflow && (ko.overflow[f] & 1);
    bool any_host = false;
    for (uint32_t r : hostonly)
      if (kw_state(r) != 0) any_host = true;
    if (first[f] == first[f + 1] && !ovf && !any_host && !fbbits) {  // no match possible
      res.status = path_ok(f) ? kPathAllowed : kNoFindings;
      return;
    }
    const std::string path(pp, pn);
    std::vector<RuleWindows> wins(R);
    std::vector<const RuleWindows*> wptr(R, nullptr);
    std::vector<uint8_t> kws(R);
    for (size_t r = 0; r < R; r++) kws[r] = kw_state(r);
    const uint64_t tk0 = prof ? __rdtsc() : 0;
    if (fbbits & 3) {
      // U+0130 / U+212A present: a keyword K1 did not see (its bit is clear; bits are exact
      // for ASCII) can only occur through one of those runes, i.e. inside a window of 3 bytes
      // per keyword letter around a rune.  Check the uncertain rules' keywords there instead
      // of over the whole file: not found -> the gate fails (0), found -> exact scan (2).
      std::vector<int64_t> runes;
      fold_rune_positions(content, n, 1 | 2, &runes);
      for (size_t r = 0; r < R; r++) {
        if (kws[r] != 3 || !rs.rules[r].kw_ascii) continue;
        bool hit = false;
        for (const auto& kw : rs.rules[r].kw_lower) {
          const int64_t span = 3 * (int64_t)kw.size();
          for (size_t i = 0; i < runes.size() && !hit; i++) {
            const int64_t a = std::max<int64_t>(0, runes[i] - span), e = std::min<int64_t>(n, runes[i] + span);
            hit = contains_fold_runes(content + a, (size_t)(e - a), kw);
          }
          if (hit) break;
        }
        kws[r] = hit ? 3 : 0;  // 3 -> whole-file exact resolution below
      }
    }
    if (prof) slots[tid].cyc[5] += __rdtsc() - tk0;
    if (ovf) {
      for (size_t r = 0; r < R; r++) {
        wins[r].whole = true;
        wptr[r] = &wins[r];
      }
    }
    for (uint32_t r : hostonly)
      if (kws[r] != 0) {
        wins[r].whole = true;
        wptr[r] = &wins[r];
      }
    // every match start lies in [end - winback, end] of some candidate end offset; the
    // reverse DFA narrows that to [leftmost start, end] or drops the candidate.  K2's end of
    // a prefix-cut program is the end of the prefix, and rule_winback the prefix's longest
    // match; the fold-rune DFAs below run whole programs, so their ends are match ends
    // (full_end) and get the whole rule's bound instead.
    auto add_end = [&](RuleWindows& w, uint32_t r, int64_t end, bool full_end) {
      int64_t lo;
      if (const DFA* rev = plan.rule_rev[r].get()) {
        lo = reverse_match_start(*rev, content, end);
        if (lo < 0) return;
        lo = align_rune(content, n, lo);
      } else {
        const int64_t back = full_end && plan.rule_atoms[r] >= 0 ? plan.rule_maxlen[r] : plan.rule_winback[r];
        lo = back < 0 ? 0 : align_rune(content, n, std::max<int64_t>(0, end - back));
      }
      w.iv.push_back({lo, end});
    };
    auto normalize = [](RuleWindows& w) {  // sort, merge touching windows
      std::sort(w.iv.begin(), w.iv.end());
      size_t o = 0;
      for (size_t i = 0; i < w.iv.size(); i++) {
        if (o && w.iv[i].first <= w.iv[o - 1].second + 1)
          w.iv[o - 1].second = std::max(w.iv[o - 1].second, w.iv[i].second);
        else
          w.iv[o++] = w.iv[i];
      }
      w.iv.resize(o);
    };
    std::sort(cand.begin() + first[f], cand.begin() + first[f + 1], by_rule_end);
    for (uint32_t k = first[f]; k < first[f + 1];) {
      uint32_t r = cand[k].rule;
      uint32_t e = k;
      while (e < first[f + 1] && cand[e].rule == r) e++;
      RuleWindows& w = wins[r];
      wptr[r] = &w;
      if (!w.whole) {
        for (uint32_t j = k; j < e && !w.whole; j++) {
          if (cand[j].end == kCandWhole) {
            w.whole = true;
            w.iv.clear();
          } else {
            add_end(w, r, cand[j].end, false);
          }
        }
        normalize(w);
      }
      k = e;
    }
    const uint64_t tf0 = prof ? __rdtsc() : 0;
    uint64_t tdfa = 0;
    if (fbbits & 6) {
      // The windows and whole-file runs below are only needed for rules whose keyword gate
      // passes.  A gate K1 left to the host (kws 2: an adapted hot keyword such as "key")
      // is settled exactly first, as scan_file would (scanner.go:164-176): random binary
      // blobs hold folding-rune byte pairs but rarely the keyword.
      std::map<std::string, bool> kwhit;
      for (size_t r = 0; r < R; r++) {
        if (kws[r] != 2 || !rs.rules[r].kw_ascii || rs.rules[r].kw_lower.empty()) continue;
        bool hit = false;
        for (const auto& kw : rs.rules[r].kw_lower) {
          auto it = kwhit.find(kw);
          if (it == kwhit.end())
            it = kwhit.emplace(kw, (fbbits & 3) ? contains_fold_runes(content, (size_t)n, kw)
                                                : contains_fold_ascii(content, (size_t)n, kw)).first;
          if ((hit = it->second)) break;
        }
        if (!hit) kws[r] = 0;
      }
      // U+212A / U+017F join ASCII letters under (?i), which the K1 anchors (literal
      // automaton, token-run counters) do not see: a match the kernels may have missed
      // contains one of them, so its start lies within rule_maxlen bytes before it.  A
      // rule without that bound runs its K2 DFA over the file here when its GPU program is
      // exact (relaxed programs leave these runes out of their sets), else the whole file.
      std::vector<int64_t> fold;
      fold_rune_positions(content, n, 2 | 4, &fold);
      // the unbounded rules in one pass of their combined fold DFA: threads injected up to
      // the last rune and followed until they die; an end before the first rune belongs to
      // a match without one (the kernels' candidates cover those)
      std::vector<uint8_t> done(R, 0);
      if (plan.fold_all_dfa && !fold.empty()) {
        const DFA& fd = *plan.fold_all_dfa;
        const size_t nf = plan.fold_rules.size();
        std::vector<uint8_t> want(nf, 0);
        bool any = false;
        for (size_t k = 0; k < nf; k++) {
          const uint32_t r = plan.fold_rules[k];
          want[k] = !(kws[r] == 0 || kws[r] == 3 || wins[r].whole);
          any |= want[k] != 0;
        }
        if (any) {
          const uint64_t td = prof ? __rdtsc() : 0;
          const int64_t q0 = fold.front(), q1 = fold.back();
          // (true: the tail past the last rune reached a state whose threads never die,
          // e.g. a (?s).* rule, and stopped there: its later ends are unknown, so every
          // wanted rule is resolved over the whole file instead)
          const bool cut = run_segment(fd, content, 0, (uint64_t)n, 0, (uint64_t)std::min<int64_t>(n, q1 + 1), ~0u,
                      [&](uint32_t mi, uint64_t pos) {
                        if ((int64_t)pos < q0) return;
                        const auto& m = fd.masks[mi];
                        for (size_t k = 0; k < nf; k++)
                          if (want[k] && ((m[k / 64] >> (k % 64)) & 1))
                            add_end(wins[plan.fold_rules[k]], plan.fold_rules[k], (int64_t)pos, true);
                      });
          if (prof) tdfa += __rdtsc() - td;
          for (size_t k = 0; k < nf; k++)
            if (want[k]) {
              const uint32_t r = plan.fold_rules[k];
              done[r] = 1;
              wptr[r] = &wins[r];
              if (cut) {
                wins[r].whole = true;
                wins[r].iv.clear();
              } else {
                normalize(wins[r]);
              }
            }
        }
      }
      for (size_t r = 0; r < R; r++) {
        if (done[r] || kws[r] == 0 || kws[r] == 3 || !rs.rules[r].regex || wins[r].whole || fold.empty()) continue;
        RuleWindows& w = wins[r];
        wptr[r] = &w;
        const int64_t ml = plan.rule_maxlen[r];
        if (ml >= 0) {
          for (int64_t q : fold) w.iv.push_back({align_rune(content, n, std::max<int64_t>(0, q - ml)), q});
        } else if (const DFA* fd = plan.rule_fold_dfa[r].get()) {
          // relaxed rule: its fold-rune DFA (a superset that accepts the runes) gives the
          // candidate ends over the file
          w.iv.clear();
          const uint64_t td = prof ? __rdtsc() : 0;
          run_segment(*fd, content, 0, (uint64_t)n, 0, (uint64_t)n, ~0u, [&](uint32_t mi, uint64_t pos) {
            if (fd->masks[mi][0] & 1) add_end(w, (uint32_t)r, (int64_t)pos, true);
          });
          if (prof) tdfa += __rdtsc() - td;
        } else if (plan.rule_group[r] >= 0 && plan.rule_relax[r] < 0) {
          // only an unrelaxed GPU program keeps U+017F / U+212A in its (?i) sets (relaxed
          // ones drop them, goregex.cpp Compiler::rune): a relaxed rule is resolved whole
          const GroupPlan& g = plan.groups[plan.rule_group[r]];
          size_t local = 0;
          while (g.rules[local] != r) local++;
          const DFA& d = *g.dfa;
          w.iv.clear();
          const uint64_t td = prof ? __rdtsc() : 0;
          run_segment(d, content, 0, (uint64_t)n, 0, (uint64_t)n, ~0u, [&](uint32_t mi, uint64_t pos) {
            if ((d.masks[mi][local / 64] >> (local % 64)) & 1) add_end(w, (uint32_t)r, (int64_t)pos, true);
          });
          if (prof) tdfa += __rdtsc() - td;
        } else {
          w.whole = true;
          w.iv.clear();
          continue;
        }
        normalize(w);
      }
    }
    if (prof) {
      slots[tid].cyc[6] += __rdtsc() - tf0 - tdfa;
      slots[tid].cyc[7] += tdfa;
    }
    // a rule whose keyword gate is uncertain and that the kernels did not scan (its
    // keyword bits were clear) is resolved over the whole file when the exact gate passes
    for (size_t r = 0; r < R; r++)
      if (kws[r] == 3) {
        kws[r] = 2;
        wins[r].whole = true;
        wptr[r] = &wins[r];
      }
    if (getenv("TSG_DEBUG_RESOLVE"))
      for (size_t r = 0; r < R; r++)
        if (wptr[r]) {
          fprintf(stderr, "file %u rule %s kws %d whole %d:", f, rs.rules[r].id.c_str(), kws[r], (int)wptr[r]->whole);
          for (auto& iv : wptr[r]->iv) fprintf(stderr, " [%ld,%ld]", (long)iv.first, (long)iv.second);
          fprintf(stderr, "\n");
        }
    FileGate gate;
    gate.kw_state = kws.data();
    gate.windows = wptr.data();
    gate.path_allowed = path_ok(f) ? 1 : 0;
    gate.ascii_fold_exact = (fbbits & 3) == 0;
    if (prof)
      for (size_t r = 0; r < R; r++)
        if (wptr[r] && (wptr[r]->whole || (!wptr[r]->iv.empty() && wptr[r]->iv[0].first == 0))) {
          n_whole++;
          if (getenv("TSG_PROF2") && n_whole < 40)
            fprintf(stderr, "whole-prefix: file %u rule %s n=%ld whole=%d iv0=[%ld,%ld] niv=%zu\n", f, rs.rules[r].id.c_str(), (long)n,
                    (int)wptr[r]->whole, wptr[r]->iv.empty() ? -1L : (long)wptr[r]->iv[0].first,
                    wptr[r]->iv.empty() ? -1L : (long)wptr[r]->iv[0].second, wptr[r]->iv.size());
        }
    const uint64_t ts0 = prof ? __rdtsc() : 0;
    scan_file(rs, path, content, (size_t)n, &gate, &res);
    if (prof) slots[tid].cyc[4] += __rdtsc() - ts0;
  });
  if (prof) {
    uint64_t t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (const auto& sl : slots)
      for (int k = 0; k < 8; k++) t[k] += sl.cyc[k];
    fprintf(stderr, "resolve: parallel part %.1f Mcyc wall; thread Mcyc: no-candidate files %.1f, candidate files %.1f "
            "(%lu files, %ld whole-prefix rule scans; scan_file %.1f), other %.1f\n",
            (__rdtsc() - t_par0) / 1e6, t[0] / 1e6, t[1] / 1e6, (unsigned long)t[3], (long)n_whole, t[4] / 1e6,
            t[2] / 1e6);
    fprintf(stderr, "resolve: fold runes: keyword windows %.1f, bounded-rule windows %.1f, whole-file DFAs %.1f Mcyc\n",
            t[5] / 1e6, t[6] / 1e6, t[7] / 1e6);
  }
}

// Start offsets of the folding runes selected by `which` (1: U+0130 = C4 B0, 2: U+212A =
// E2 84 AA, 4: U+017F = C5 BF), in order.  SSE2 finds their lead bytes 16 at a time.
void fold_rune_positions(const uint8_t* s, int64_t n, uint32_t which, std::vector<int64_t>* out) {
  out->clear();
  const __m128i c4 = _mm_set1_epi8((char)0xC4), c5 = _mm_set1_epi8((char)0xC5), e2 = _mm_set1_epi8((char)0xE2);
  auto check = [&](int64_t q) {
    if ((which & 1) && s[q] == 0xC4 && q + 1 < n && s[q + 1] == 0xB0) out->push_back(q);
    else if ((which & 4) && s[q] == 0xC5 && q + 1 < n && s[q + 1] == 0xBF) out->push_back(q);
    else if ((which & 2) && s[q] == 0xE2 && q + 2 < n && s[q + 1] == 0x84 && s[q + 2] == 0xAA) out->push_back(q);
  };
  int64_t q = 0;
  for (; q + 16 <= n; q += 16) {
    const __m128i b = _mm_loadu_si128((const __m128i*)(s + q));
    uint32_t bits = (uint32_t)_mm_movemask_epi8(
        _mm_or_si128(_mm_or_si128(_mm_cmpeq_epi8(b, c4), _mm_cmpeq_epi8(b, c5)), _mm_cmpeq_epi8(b, e2)));
    while (bits) {
      check(q + __builtin_ctz(bits));
      bits &= bits - 1;
    }
  }
  for (; q < n; q++) check(q);
}
}  // namespace tsg
