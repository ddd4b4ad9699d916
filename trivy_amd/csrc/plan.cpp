// GPU plan construction: build_plan and its passes, and the plan digest.
#include "plan.hpp"
#include "internal.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <unordered_map>
#include <unordered_set>
#include <set>
#include <thread>
#include <type_traits>

namespace tsg {

static std::string ascii_lower(std::string s) {
  for (char& c : s)
    if (c >= 'A' && c <= 'Z') c = (char)(c + 32);
  return s;
}

static bool is_ascii(const std::string& s) {
  for (unsigned char c : s)
    if (c >= 0x80) return false;
  return true;
}

// 4-byte strings frequent in source text (common4.inc): a K1X window on one of them costs a
// verify record per occurrence
static const std::unordered_set<uint32_t>& common4() {
  static const std::unordered_set<uint32_t> set = [] {
    static const char kCommon4[][5] = {
#include "common4.inc"
    };
    std::unordered_set<uint32_t> s;
    for (const auto& g : kCommon4) s.insert(x_prefix4((const uint8_t*)g));
    return s;
  }();
  return set;
}

// K1X windows of every literal of the plan: per literal the offset j0 whose windows hold
// the fewest common 4-grams, then are shared by the fewest other literals (a window shared
// by k literals costs k verifications per hit: 100 `begin_<name>` anchors all starting
// "begi" made every "-----BEGIN" line of a batch check 100 literals).
static void x_place_windows(Plan* p, int step) {
  std::unordered_map<uint32_t, uint32_t> mult;
  for (const auto& l : p->x_lits) {
    std::unordered_set<uint32_t> mine;
    for (size_t j = 0; j + 4 <= l.size(); j++) mine.insert(x_prefix4((const uint8_t*)l.data() + j));
    for (uint32_t g : mine) mult[g]++;
  }
  p->x_j0.assign(p->x_lits.size(), 0);
  for (size_t i = 0; i < p->x_lits.size(); i++) {
    const std::string& l = p->x_lits[i];
    const size_t last = std::min(l.size() - 3 - (size_t)step, (size_t)256 - (size_t)step);
    uint64_t best = UINT64_MAX;
    for (size_t j = 0; j <= last; j++) {
      uint64_t c = 0;
      for (size_t t = j; t < j + (size_t)step; t++) {
        const uint32_t g = x_prefix4((const uint8_t*)l.data() + t);
        c += (common4().count(g) ? 1000000u : 0u) + mult[g];
      }
      if (c < best) {
        best = c;
        p->x_j0[i] = (uint8_t)j;
      }
    }
  }
}

// K1X windows of a lowercased literal at step `step`: the first offset j0 whose windows
// j0 .. j0 + step - 1 hold the fewest common 4-grams.  Returns that count (0: a quiet
// literal), -1 when the literal is too short for the step.
static int x_pick(const std::string& l, int step, uint32_t* j0) {
  if (l.size() < (size_t)step + 3) return -1;
  const size_t last = std::min(l.size() - 3 - (size_t)step, (size_t)256 - (size_t)step);
  int best = -1;
  for (size_t j = 0; j <= last && best != 0; j++) {
    int c = 0;
    for (size_t t = j; t < j + (size_t)step; t++) c += common4().count(x_prefix4((const uint8_t*)l.data() + t)) ? 1 : 0;
    if (best < 0 || c < best) {
      best = c;
      *j0 = (uint32_t)j;
    }
  }
  return best;
}

namespace {

bool in_set(const uint64_t* set, const uint8_t* cls, int bit) {
  for (int c = 0; c < 128; c++)
    if (((set[c >> 6] >> (c & 63)) & 1) && !((cls[c] >> bit) & 1)) return false;
  return true;
}

struct Anchor {
  uint32_t kind = kEvAlways;  // kEvRunU, kEvRunD, kEvLit0 (literal), kEvAlways
  std::string lit;
  int first_atom = 0;
  int64_t evdist = 0;
  std::string desc = "none";
};

// The event every match of a rule must contain, preferring long class runs (the secret
// part of nearly every rule) over literals: the keyword gate already handles rare
// literals, and common ones ("key", "sk", "-----") would put events everywhere.  A rule
// without keywords (every file gated) takes a long literal first when it has one (score
// >= 6, e.g. a 5-byte name): token runs are common, its literal is not.
Anchor choose_anchor(const Regexp& re, const Plan& p, bool literal_first) {
  const std::vector<AtomInfo> at = re.Atoms();
  const int n = (int)at.size();
  std::vector<int64_t> B(n + 1, 0);
  for (int i = 0; i < n; i++)
    B[i + 1] = (B[i] < 0 || at[i].max_bytes < 0) ? -1 : B[i] + at[i].max_bytes;
  Anchor best;
  auto take = [&](uint32_t kind, int t, int64_t len, const std::string& lit, const char* what) {
    Anchor a;
    a.kind = kind;
    a.lit = lit;
    if (B[t] >= 0) {
      a.first_atom = 0;
      a.evdist = B[t] + len - 1;
    } else {
      a.first_atom = t;  // unbounded prefix: the GPU program is the suffix from the anchor
      a.evdist = len - 1;
    }
    a.desc = std::string(what) + (lit.empty() ? "" : " '" + lit + "'") + " at atom " +
             std::to_string(t) + (a.first_atom ? " (suffix)" : "");
    return a;
  };
  double best_score = 0;
  auto best_literal = [&]() {
    for (int i = 0; i < n;) {
      if (at[i].lit < 0) {
        i++;
        continue;
      }
      int j = i;
      std::string s;
      double score = 0;
      while (j < n && at[j].lit >= 0) {
        int c = at[j].lit;
        if (s.size() < 24) {
          s.push_back((char)c);
          score += (c >= 'a' && c <= 'z') ? 1.0 : (c >= '0' && c <= '9') ? 1.3 : 1.6;
        }
        j++;
      }
      if (score >= 3.0 && score > best_score) {
        best_score = score;
        best = take(1u << kEvLit0, i, (int64_t)s.size(), s, "literal");
      }
      i = j;
    }
  };
  if (literal_first) {
    best_literal();
    if (best_score >= 6.0) return best;
    best = Anchor();
    best_score = 0;
  }
  for (int bit = 0; bit < 2; bit++) {
    const int k = p.run_k[bit];
    for (int i = 0; i < n;) {
      if (!(at[i].ascii_only && in_set(at[i].set, p.run_cls, bit))) {
        i++;
        continue;
      }
      int j = i;
      int64_t run = 0;
      while (j < n && at[j].ascii_only && in_set(at[j].set, p.run_cls, bit)) run += at[j++].min_bytes;
      if (run >= k) return take(bit == 0 ? kEvRunU : kEvRunD, i, k, "", bit == 0 ? "run U" : "run D");
      i = j;
    }
  }
  best_literal();
  return best;
}

// Inject-mode states of the union of two DFAs' searches, counted as the reachable pairs
// of their product (each union state is a pair of component states), up to `cap`.  A
// lower bound on the states a subset construction of the merged programs builds, so
// "> cap" rejects a merge without building it.
size_t product_states(const DFA& a, const DFA& b, size_t cap) {
  std::vector<uint8_t> seen((size_t)a.nstates * b.nstates, 0);
  std::vector<std::pair<uint32_t, uint32_t>> stack;
  uint16_t pcls[256][2];
  int np = 0;
  {
    std::map<std::pair<int, int>, int> idx;
    for (int c = 0; c < 256; c++) {
      auto k = std::make_pair((int)a.cls[c], (int)b.cls[c]);
      if (!idx.count(k)) idx[k] = np++;
      pcls[c][0] = (uint16_t)a.cls[c];
      pcls[c][1] = (uint16_t)b.cls[c];
    }
  }
  std::vector<int> rep;  // one byte per joint class
  {
    std::set<std::pair<int, int>> done;
    for (int c = 0; c < 256; c++)
      if (done.insert({pcls[c][0], pcls[c][1]}).second) rep.push_back(c);
  }
  size_t n = 0;
  auto push = [&](uint32_t x, uint32_t y) {
    uint8_t& v = seen[(size_t)x * b.nstates + y];
    if (v) return;
    v = 1;
    n++;
    stack.push_back({x, y});
  };
  for (int c = 0; c < 4; c++) push(a.start[c], b.start[c]);
  while (!stack.empty() && n <= cap) {
    auto [x, y] = stack.back();
    stack.pop_back();
    for (int c : rep) push(a.next[(size_t)x * a.nclasses + pcls[c][0]], b.next[(size_t)y * b.nclasses + pcls[c][1]]);
  }
  return n;
}

// Table bytes of a literal automaton: its states are the literals' distinct prefixes (and
// the root), its classes at most the distinct bytes + 1.  (Every literal that reaches it is
// lowercase already: keywords are lowered when the rules are compiled, AtomInfo::lit is.)
struct TrieCost {
  std::set<std::string> pre;
  bool bytes[256] = {false};
  size_t nbytes = 0;
  // rows x (classes + pad) x 2 with literal s added ("": as it stands)
  size_t with(const std::string& s, size_t pad) const {
    size_t npre = 0, nb = 0;
    bool seen[256] = {false};
    for (size_t i = 1; i <= s.size(); i++) npre += pre.count(s.substr(0, i)) ? 0 : 1;
    for (unsigned char ch : s) {
      if (!bytes[ch] && !seen[ch]) nb++;
      seen[ch] = true;
    }
    return (pre.size() + npre + 1) * (nbytes + nb + 1 + pad) * 2;
  }
  void add(const std::string& s) {
    for (size_t i = 1; i <= s.size(); i++) pre.insert(s.substr(0, i));
    for (unsigned char ch : s) {
      if (!bytes[ch]) nbytes++;
      bytes[ch] = true;
    }
  }
};

// milliseconds since the last call (TSG_PROF lines)
struct Lap {
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  double ms() {
    const auto t0 = t;
    t = std::chrono::steady_clock::now();
    return std::chrono::duration<double, std::milli>(t - t0).count();
  }
};

// build_plan's passes, in the order it runs them, and what crosses from one to the next.
struct PlanBuild {
  const Ruleset& rs;
  const PlanOptions& opt;
  Plan* const p;
  const size_t R;
  // rules are independent in the per-rule passes: they run on the shared pool
  const int threads = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  const bool prof = getenv("TSG_PROF") != nullptr, prof2 = getenv("TSG_PROF2") != nullptr;
  DFAOptions one;  // of every K2 DFA
  std::vector<std::string> kws;              // number_keywords -> choose_k1: keyword id -> its bytes
  std::vector<Anchor> anchor;                // rule_programs -> choose_k1
  std::vector<std::unique_ptr<DFA>> single;  // rule_programs -> pack_groups, which moves them out
  // choose_k1, what is not in the automaton: keywords left out of K1 (table budget; a literal
  // no ASCII text contains holds their id), and in hashed mode (K1X) the keywords and anchors
  // that leave it
  std::vector<char> kw_dropped, kw_hashed, anchor_hashed;
  std::vector<char> litg;  // per group: its event is an anchor literal

  PlanBuild(const Ruleset& rs, const PlanOptions& opt, Plan* p)
      : rs(rs), opt(opt), p(p), R(rs.rules.size()), anchor(R), single(R) {
    one.max_states = opt.max_group_states;
  }

  bool fits(const DFA& d, size_t nrules) const {
    return d.nstates <= opt.max_group_states &&
           (size_t)d.nstates * d.nclasses * 2 <= (size_t)opt.max_group_table_bytes &&
           (int)nrules <= opt.max_rules_per_group;
  }

  void group_kwmask(GroupPlan& g) const {
    g.kwmask.assign(p->kw_words, 0);
    for (uint32_t r : g.rules) {
      if (p->rule_kw_mode[r] != kKwBits) {
        g.always = true;
        continue;
      }
      for (uint32_t k : p->rule_kws[r]) g.kwmask[k / 32] |= 1u << (k % 32);
    }
    // (the folding-rune pseudo keywords gate nothing here: a file holding one is always
    // resolved on the host, which scans its uncertain-keyword rules whole and adds windows
    // before the runes that (?i) folds, whatever K2 found)
  }

  // ---- keywords (Rule.MatchKeywords, scanner.go:164-176)
  void number_keywords() {
    std::map<std::string, uint32_t> kwid;
    for (size_t r = 0; r < R; r++) {
      const RuleC& rule = rs.rules[r];
      if (rule.kw_lower.empty()) continue;
      bool ascii = true;
      for (const auto& k : rule.kw_lower) ascii &= is_ascii(k);
      if (!ascii) {
        p->rule_kw_mode[r] = kKwUnknown;
        continue;
      }
      p->rule_kw_mode[r] = kKwBits;
      for (const auto& k : rule.kw_lower) {
        auto it = kwid.find(k);
        uint32_t id;
        if (it == kwid.end()) {
          id = (uint32_t)kws.size();
          kwid[k] = id;
          kws.push_back(k);
        } else {
          id = it->second;
        }
        p->rule_kws[r].push_back(id);
      }
    }
    p->fb_kw0 = (int)kws.size();
    kws.push_back("\xc4\xb0");      // U+0130, bytes.ToLower -> "i"
    kws.push_back("\xe2\x84\xaa");  // U+212A, bytes.ToLower -> "k"; (?i)k folds to it
    kws.push_back("\xc5\xbf");      // U+017F, (?i)s folds to it
    p->n_kw = (int)kws.size();
    p->kw_words = (p->n_kw + 31) / 32;
    for (const auto& k : kws) p->kw_len.push_back((uint16_t)std::min<size_t>(k.size(), 0xFFFF));
  }

  // ---- per rule: anchor event and GPU program
  void rule_program(size_t r) {
    const RuleC& rule = rs.rules[r];
    if (!rule.regex) return;
    p->rule_maxlen[r] = max_match_len(rule.regex->prog());
    anchor[r] = choose_anchor(*rule.regex, *p, rule.kw_lower.empty());
    const int fa = anchor[r].first_atom;
    // the program relaxed to k and cut to its first t atoms (-1: all), kept if its DFA fits
    auto attempt = [&](int k, int t) {
      Prog pr = (k < 0 && fa == 0) ? rule.regex->prog() : rule.regex->RelaxedProg(k, t, fa);
      std::string e;
      auto d = build_dfa({&pr}, one, &e);
      if (!d || !fits(*d, 1)) return false;
      single[r] = std::move(d);
      p->rule_relax[r] = k;
      p->rule_atoms[r] = t;
      p->rule_prog[r] = std::move(pr);
      return true;
    };
    // exact program first, then ever stronger relaxations of counted repetitions, then
    // ever shorter prefixes of the top-level concatenation
    for (int k : {-1, 32, 16, 8, 4, 2, 1, 0})
      if (attempt(k, -1)) break;
    for (int t = rule.regex->NumAtoms() - fa - 1; !single[r] && t >= 1; t--)
      for (int k : {8, 2, 0})
        if (attempt(k, t)) break;
    if (!single[r]) {
      p->rule_hostonly[r] = 1;
      return;
    }
    // where a GPU end offset e lets the exact match start
    if (fa > 0) {
      p->rule_winback[r] = -1;
    } else if (p->rule_atoms[r] >= 0) {
      p->rule_winback[r] = max_match_len(rule.regex->RelaxedProg(-1, p->rule_atoms[r]));
    } else {
      p->rule_winback[r] = p->rule_maxlen[r];
    }
    p->rule_event[r] = anchor[r].kind;
    p->rule_evdist[r] = anchor[r].evdist;
    p->rule_first_atom[r] = fa;
    p->rule_anchor[r] = anchor[r].desc;
  }

  // ---- K2 rule groups: greedy packing under the state / table caps, among rules with
  // the same kind of event (their windows coincide)
  void pack_groups() {
    for (uint32_t kind : {kEvRunU, kEvRunD, 1u << kEvLit0, kEvAlways}) {
      std::vector<uint32_t> cur;
      std::unique_ptr<DFA> cur_dfa;
      auto flush = [&]() {
        if (cur.empty()) return;
        GroupPlan g;
        g.dfa = std::move(cur_dfa);
        g.rules = cur;
        group_kwmask(g);
        g.events = kind;
        g.evdist = 0;
        for (uint32_t r : cur) {
          p->rule_group[r] = (int)p->groups.size();
          g.evdist = std::max(g.evdist, p->rule_evdist[r]);
        }
        p->groups.push_back(std::move(g));
        cur.clear();
      };
      for (size_t r = 0; r < R; r++) {
        if (!single[r] || p->rule_event[r] != kind) continue;
        // two programs whose DFAs together exceed the cap have not merged under it on any
        // rule set measured (unanchored searches share few states): skip the construction
        std::unique_ptr<DFA> merged;
        if (!cur.empty() && cur_dfa->nstates + single[r]->nstates <= opt.max_group_states &&
            product_states(*cur_dfa, *single[r], opt.max_group_states) <= (size_t)opt.max_group_states) {
          std::vector<const Prog*> progs;
          for (uint32_t q : cur) progs.push_back(&p->rule_prog[q]);
          progs.push_back(&p->rule_prog[r]);
          std::string e;
          merged = build_dfa(progs, one, &e);
          const bool ok = merged && fits(*merged, cur.size() + 1);
          if (prof2)
            fprintf(stderr, "merge %d+%d (nc %d,%d) -> %d %s\n", cur_dfa->nstates, single[r]->nstates,
                    cur_dfa->nclasses, single[r]->nclasses, merged ? merged->nstates : -1, ok ? "ok" : "FAIL");
          if (!ok) merged.reset();
        }
        if (!merged) flush();
        cur.push_back((uint32_t)r);
        cur_dfa = merged ? std::move(merged) : std::move(single[r]);
      }
      flush();
    }
  }

  // ---- K1 automaton: keywords + anchor literals; literal groups share event bits.  Builds
  // it from what kw_dropped / kw_hashed / anchor_hashed leave in; false: over the table budget.
  bool build_k1(bool with_anchors) {
    std::vector<std::string> lits = kws;
    for (size_t k = 0; k < lits.size(); k++)
      if (kw_dropped[k] || kw_hashed[k]) lits[k] = never_literal();
    std::map<std::string, std::pair<int32_t, uint32_t>> xl;  // K1X literal -> keyword id, events
    for (size_t k = 0; k < kws.size(); k++)
      if (kw_hashed[k]) xl[ascii_lower(kws[k])] = {(int32_t)k, 0u};
    std::vector<uint32_t> lit_event(lits.size(), 0);
    std::map<std::string, uint32_t> lid;
    for (size_t i = 0; i < lits.size(); i++) lid.emplace(lits[i], (uint32_t)i);
    int nlitgroups = 0;
    for (size_t gi = 0; gi < p->groups.size(); gi++) {
      GroupPlan& g = p->groups[gi];
      if (!litg[gi]) continue;
      if (!with_anchors) {
        g.events = kEvAlways;
        for (uint32_t r : g.rules) p->rule_event[r] = kEvAlways;
        continue;
      }
      const uint32_t bit = 1u << (kEvLit0 + (nlitgroups++ % kEvLitBits));
      g.events = bit;
      for (uint32_t r : g.rules) {
        p->rule_event[r] = bit;
        const std::string& s = anchor[r].lit;
        if (anchor_hashed[r]) {
          auto xi = xl.find(ascii_lower(s));
          if (xi == xl.end()) xl[ascii_lower(s)] = {-1, bit};
          else xi->second.second |= bit;
          continue;
        }
        auto it = lid.find(s);
        uint32_t id;
        if (it == lid.end()) {
          id = (uint32_t)lits.size();
          lid.emplace(s, id);
          lits.push_back(s);
          lit_event.push_back(0);
        } else {
          id = it->second;
        }
        lit_event[id] |= bit;
      }
    }
    DFAOptions o;
    o.max_states = 32767;
    o.with_noinject = false;
    std::string e;
    auto d = build_keyword_dfa(lits, o, &e);
    if (!d) return false;
    if ((size_t)d->nstates * d->nclasses * 2 > (size_t)opt.max_kw_table_bytes) return false;
    p->n_lit = (int)lits.size();
    p->lit_event = lit_event;
    p->k1_lits = lits;
    p->kw_mask_events.assign(d->masks.size(), 0);
    for (size_t m = 0; m < d->masks.size(); m++)
      for (int id = 0; id < p->n_lit; id++)
        if ((d->masks[m][id / 64] >> (id % 64)) & 1) p->kw_mask_events[m] |= lit_event[id];
    size_t longest = 0;
    for (const auto& s : lits) longest = std::max(longest, s.size());
    int w = (int)std::max<size_t>(longest, (size_t)std::max(p->run_k[0], p->run_k[1]));
    p->warm = (w - 1 + 15) / 16 * 16;
    p->kw_dfa = std::move(d);
    p->x_lits.clear();
    p->x_kw.clear();
    p->x_event.clear();
    p->x_j0.clear();
    for (const auto& kv : xl) {
      p->x_lits.push_back(kv.first);
      p->x_kw.push_back(kv.second.first);
      p->x_event.push_back(kv.second.second);
    }
    return true;
  }

  // estimated table bytes of the automaton over the keywords (and anchors) left in
  size_t k1_estimate(bool with_anchors) const {
    TrieCost in;
    for (size_t k = 0; k < kws.size(); k++)
      if (!kw_dropped[k] && !kw_hashed[k]) in.add(kws[k]);
    if (with_anchors)
      for (size_t r = 0; r < R; r++)
        if (!anchor[r].lit.empty() && !anchor_hashed[r]) in.add(anchor[r].lit);
    return in.with("", 0);
  }

  // The automaton with the anchor literals, else without them (their groups then listen to
  // every chunk).  gate_with / gate_without: an estimate far over the budget skips that
  // exact build.
  bool k1_with_anchors_else_without(bool gate_with, bool gate_without) {
    auto k1 = [&](bool with_anchors, bool gate) {
      if (gate && k1_estimate(with_anchors) > 4 * (size_t)opt.max_kw_table_bytes) return false;
      return build_k1(with_anchors);
    };
    return k1(true, gate_with) || k1(false, gate_without);
  }

  // K1X at one step: samples one 4-byte window every `step` bytes, so it takes literals of
  // step + 3 bytes or more; the shorter ones stay in the automaton, and the others fill what
  // is left of a packed table (k1_packed_fits) in rule order -- the builtin rules' first
  // (scanner.go:302-311), whose keywords are the ones common in real text -- the rest are
  // hashed.  Keyword bits stay exact, anchors keep their events.
  void k1x_assign(int step) {
    const size_t xmin = (size_t)step + 3;
    TrieCost in;
    std::fill(kw_hashed.begin(), kw_hashed.end(), 0);
    std::fill(anchor_hashed.begin(), anchor_hashed.end(), 0);
    for (size_t k = 0; k < kws.size(); k++)
      if (!kw_dropped[k] && kws[k].size() < xmin) in.add(kws[k]);
    for (size_t r = 0; r < R; r++)
      if (!anchor[r].lit.empty() && anchor[r].lit.size() < xmin) in.add(anchor[r].lit);
    // two passes in rule order: literals whose every K1X window choice holds a 4-gram
    // common in text first, then the quiet ones
    for (int pass = 0; pass < 2; pass++) {
      std::vector<char> kw_seen(kws.size(), 0);
      auto place = [&](const std::string& s, char* hashed) {
        uint32_t j0 = 0;
        const int c = x_pick(ascii_lower(s), step, &j0);
        if (c < 0 || (pass == 0) != (c > 0)) return;  // too short (kept above), or the other pass
        // (classes padded to 2 mod 4: an upper bound of the exact automaton's table)
        if (in.with(s, 3) <= 65536) in.add(s);
        else *hashed = 1;
      };
      for (size_t r = 0; r < R; r++) {
        for (uint32_t k : p->rule_kws[r])
          if ((int)k < p->fb_kw0 && !kw_dropped[k] && !kw_seen[k]) {
            kw_seen[k] = 1;
            place(kws[k], &kw_hashed[k]);
          }
        if (!anchor[r].lit.empty()) place(anchor[r].lit, &anchor_hashed[r]);
      }
      for (int k = 0; k < p->fb_kw0; k++)  // keywords no rule lists (none today)
        if (!kw_seen[k] && !kw_dropped[k]) place(kws[k], &kw_hashed[k]);
    }
  }

  // Too many literal bytes for an LDS-resident automaton (large user rule sets): the widest
  // step whose automaton fits the packed table, else the widest that builds (the x_step test
  // knob forces one)
  bool k1x_split() {
    const int forced = knobs().x_step.load();
    for (int attempt = 0; attempt < 6; attempt++) {
      const int step = (attempt % 3 == 0) ? 4 : (attempt % 3 == 1) ? 2 : 1;
      const bool need_packed = attempt < 3;
      if (forced && step != forced) continue;
      k1x_assign(step);
      if (!k1_with_anchors_else_without(true, true)) continue;
      if (need_packed && !forced && (size_t)p->kw_dfa->nstates * p->kw_dfa->nclasses * 2 > 65536) continue;
      p->x_step = step;
      x_place_windows(p, step);
      return true;
    }
    std::fill(kw_hashed.begin(), kw_hashed.end(), 0);
    std::fill(anchor_hashed.begin(), anchor_hashed.end(), 0);
    return false;
  }

  // Too many keyword bytes for an LDS-resident automaton (large user rule sets): leave
  // keywords out, longest first (they cost the most states), until it fits.  Their rules
  // get the exact keyword gate on the host, and their groups are scanned on every file.
  bool k1_drop_keywords() {
    std::vector<int> order;
    for (int k = 0; k < p->fb_kw0; k++) order.push_back(k);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return kws[a].size() > kws[b].size(); });
    // Estimate first, so the exact build runs once or twice.
    size_t next = 0;
    while (next < order.size() && k1_estimate(false) > (size_t)opt.max_kw_table_bytes) {
      const size_t m = std::max<size_t>(1, (order.size() - next) / 8);
      for (size_t k = 0; k < m && next < order.size(); k++) kw_dropped[order[next++]] = 1;
    }
    bool ok = k1_with_anchors_else_without(true, false);
    while (next < order.size() && !ok) {
      for (size_t m = std::max<size_t>(1, order.size() / 32); m > 0 && next < order.size(); m--)
        kw_dropped[order[next++]] = 1;
      ok = k1_with_anchors_else_without(false, false);
    }
    if (!ok) return false;
    for (size_t r = 0; r < R; r++) {
      if (p->rule_kw_mode[r] != kKwBits) continue;
      for (uint32_t k : p->rule_kws[r])
        if (kw_dropped[k]) p->rule_kw_mode[r] = kKwUnknown;
    }
    for (auto& g : p->groups) group_kwmask(g);
    return true;
  }

  // The K1 literal choice: the whole set in the automaton, else the K1X split, else
  // keywords left out.
  bool choose_k1() {
    litg.assign(p->groups.size(), 0);
    for (size_t g = 0; g < p->groups.size(); g++) litg[g] = p->groups[g].events == (1u << kEvLit0);
    kw_dropped.assign(kws.size(), 0);
    kw_hashed.assign(kws.size(), 0);
    anchor_hashed.assign(R, 0);
    return k1_with_anchors_else_without(true, true) || (!knobs().no_k1x.load() && k1x_split()) ||
           k1_drop_keywords();
  }

  // ---- host resolver: fold-rune DFAs of the unbounded relaxed rules
  void fold_dfas() {
    p->rule_fold_dfa.resize(R);
    std::vector<Prog> fold_prog(R);
    pool_for(R, threads, [&](size_t r) {
      const RuleC& rule = rs.rules[r];
      if (!rule.regex || p->rule_relax[r] < 0 || p->rule_maxlen[r] >= 0 || p->rule_group[r] < 0) return;
      DFAOptions o;
      o.max_states = 4096;
      for (int k : {p->rule_relax[r], 8, 2, 0}) {
        Prog pr = rule.regex->RelaxedProg(k, -1, 0, true);
        std::string e;
        auto d = build_dfa({&pr}, o, &e);
        if (d) {
          p->rule_fold_dfa[r] = std::move(d);
          fold_prog[r] = std::move(pr);
          break;
        }
      }
    }, 1);
    // all unbounded rules' fold programs in one DFA (resolve_batch: one pass per file)
    std::vector<const Prog*> progs;
    for (size_t r = 0; r < R; r++) {
      if (!rs.rules[r].regex || p->rule_maxlen[r] >= 0) continue;
      if (p->rule_fold_dfa[r]) {
        progs.push_back(&fold_prog[r]);
      } else if (p->rule_group[r] >= 0 && p->rule_relax[r] < 0) {
        progs.push_back(&p->rule_prog[r]);
      } else {
        continue;
      }
      p->fold_rules.push_back((uint32_t)r);
    }
    if (progs.size() > 1) {
      DFAOptions o;
      o.max_states = 16384;
      std::string e;
      p->fold_all_dfa = build_dfa(progs, o, &e);
      if (p->fold_all_dfa) p->fold_all_dfa->pack();
    }
  }

  // ---- host resolver: reverse DFAs of the exact programs
  void reverse_dfas() {
    p->rule_rev.resize(R);
    // (only where the forward bound is loose: unbounded or long windows; the subset
    // construction of the counted generic rules would cost more than it saves)
    for (size_t r = 0; r < R; r++) {
      if (!rs.rules[r].regex || (p->rule_winback[r] >= 0 && p->rule_winback[r] <= 1024)) continue;
      // a prefix-cut program's candidate end is the end of the prefix, not of a match: the
      // whole regex run backwards from it finds nothing and would drop every candidate
      if (p->rule_atoms[r] >= 0) continue;
      DFAOptions o;
      o.max_states = 2048;
      std::string e;
      Lap lap;
      p->rule_rev[r] = build_reverse_dfa(rs.rules[r].regex->prog(), o, &e);
      if (p->rule_rev[r]) p->rule_rev[r]->pack();
      if (prof)
        fprintf(stderr, "rev %s: %d states %.1f ms\n", rs.rules[r].id.c_str(),
                p->rule_rev[r] ? p->rule_rev[r]->nstates : -1, lap.ms());
    }
  }

  // ---- Global.AllowPath automaton (exact on ASCII paths)
  void allow_path_dfa() {
    std::vector<const Prog*> paths;
    for (const auto& a : rs.allow)
      if (a.path) paths.push_back(&a.path->prog());
    if (paths.empty()) return;
    DFAOptions o;
    o.max_states = 1 << 16;
    std::string e;
    p->allow_path_dfa = build_dfa(paths, o, &e);  // may be null: exact VM is used then
  }
};

}  // namespace

std::unique_ptr<Plan> build_plan(const Ruleset& rs, const PlanOptions& opt, std::string* err) {
  auto p = std::make_unique<Plan>();
  const size_t R = rs.rules.size();
  p->rule_kw_mode.assign(R, kKwAlways);
  p->rule_kws.assign(R, {});
  p->rule_group.assign(R, -1);
  p->rule_hostonly.assign(R, 0);
  p->rule_maxlen.assign(R, -1);
  p->rule_event.assign(R, kEvAlways);
  p->rule_evdist.assign(R, 0);
  p->rule_first_atom.assign(R, 0);
  p->rule_anchor.assign(R, "none");
  p->rule_relax.assign(R, -1);
  p->rule_atoms.assign(R, -1);
  p->rule_winback.assign(R, -1);
  p->rule_prog.assign(R, Prog{});
  // run classes: U = [A-Za-z0-9+/=_.-] (secrets, tokens, base64), D = [0-9-]
  for (int c = 0; c < 256; c++) {
    bool u = (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || (c >= '0' && c <= '9') ||
             c == '+' || c == '/' || c == '=' || c == '_' || c == '.' || c == '-';
    bool d = (c >= '0' && c <= '9') || c == '-';
    p->run_cls[c] = (uint8_t)((u ? 1 : 0) | (d ? 2 : 0));
  }

  PlanBuild b(rs, opt, p.get());
  Lap lap;
  b.number_keywords();
  pool_for(R, b.threads, [&](size_t r) { b.rule_program(r); }, 1);
  if (b.prof) fprintf(stderr, "plan: per-rule DFAs %.1f ms\n", lap.ms());
  b.pack_groups();
  if (b.prof) {
    fprintf(stderr, "plan: grouping %.1f ms (%zu groups)\n", lap.ms(), p->groups.size());
    for (size_t g = 0; g < p->groups.size(); g++)
      fprintf(stderr, "plan: group %zu: %zu rules, %d states x %d classes (%zu table bytes), events %#x\n", g,
              p->groups[g].rules.size(), p->groups[g].dfa->nstates, p->groups[g].dfa->nclasses,
              (size_t)p->groups[g].dfa->nstates * p->groups[g].dfa->nclasses * 2, p->groups[g].events);
    lap.ms();
  }
  if (!b.choose_k1()) {
    if (err) *err = "keyword automaton exceeds the K1 table budget";
    return nullptr;
  }
  if (b.prof) fprintf(stderr, "plan: K1 %.1f ms\n", lap.ms());
  b.fold_dfas();
  b.reverse_dfas();
  if (b.prof) fprintf(stderr, "plan: reverse DFAs %.1f ms\n", lap.ms());
  b.allow_path_dfa();
  return p;
}

// ------------------------------------------------------------------ plan digest
namespace {

// FNV-1a over a canonical byte stream: every integer as 8 little-endian bytes (signed ones
// sign-extended), a string or vector as its length and then its elements, a fixed array as
// its elements, a unique_ptr as a 0 / 1 marker and then the object.
struct Digest {
  uint64_t h = 0xcbf29ce484222325ull;
  void raw(const void* p, size_t n) {
    for (size_t i = 0; i < n; i++) h = (h ^ ((const uint8_t*)p)[i]) * 0x100000001b3ull;
  }
  void u64(uint64_t v) {
    uint8_t b[8];
    for (int i = 0; i < 8; i++) b[i] = (uint8_t)(v >> (8 * i));
    raw(b, 8);
  }
  template <class T>
  std::enable_if_t<std::is_integral<T>::value> put(T v) {
    u64(std::is_signed<T>::value ? (uint64_t)(int64_t)v : (uint64_t)v);
  }
  void put(const std::string& s) {
    u64(s.size());
    raw(s.data(), s.size());
  }
  template <class A, class B>
  void put(const std::pair<A, B>& x) {
    put(x.first);
    put(x.second);
  }
  template <class T>
  void put(const std::vector<T>& v) {
    u64(v.size());
    for (const auto& x : v) put(x);
  }
  template <class T, size_t N>
  void put(const T (&a)[N]) {
    for (const auto& x : a) put(x);
  }
  template <class T>
  void put(const std::unique_ptr<T>& x) {
    put((uint8_t)(x ? 1 : 0));
    if (x) put(*x);
  }
  void put(const Inst& i) {
    put((uint8_t)i.op);
    put(i.out);
    put(i.arg);
  }
  void put(const Prog& p) {
    put(p.inst);
    put(p.runes);
    put(p.start);
    put(p.nslots);
    put(p.ascii);
    put(p.prefix);
  }
  void put(const DFA& d) {
    put(d.nregex);
    put(d.nstates);
    put(d.nclasses);
    put(d.mask_words);
    put(d.cls);
    put(d.next);
    put(d.acc);
    put(d.eot_acc);
    put(d.masks);
    put(d.start);
    put(d.to_noinject);
    put(d.dead);
    put(d.immortal);
    put(d.noinject);
    put(d.max_len);
    put(d.anchored);
    put(d.packed);
    put(d.need_word);
    put(d.need_nl);
    put(d.need_bot);
  }
  void put(const GroupPlan& g) {
    put(g.dfa);
    put(g.rules);
    put(g.kwmask);
    put(g.always);
    put(g.events);
    put(g.evdist);
  }
};

}  // namespace

// Every member of Plan, in declaration order (and every member of GroupPlan, DFA, Prog and
// Inst above).  A member added to one of those structs has to be added here, or the plan
// digest tests (tests/test_plan_digest.py) stop seeing changes to it.
uint64_t plan_digest(const Plan& p) {
  Digest d;
  d.put(p.kw_dfa);
  d.put(p.n_kw);
  d.put(p.n_lit);
  d.put(p.kw_words);
  d.put(p.fb_kw0);
  d.put(p.kw_mask_events);
  d.put(p.lit_event);
  d.put(p.k1_lits);
  d.put(p.kw_len);
  d.put(p.x_lits);
  d.put(p.x_kw);
  d.put(p.x_event);
  d.put(p.x_step);
  d.put(p.x_j0);
  d.put(p.run_cls);
  d.put(p.run_k);
  d.put(p.warm);
  d.put(p.rule_event);
  d.put(p.rule_evdist);
  d.put(p.rule_first_atom);
  d.put(p.rule_anchor);
  d.put(p.rule_kw_mode);
  d.put(p.rule_kws);
  d.put(p.groups);
  d.put(p.rule_group);
  d.put(p.rule_hostonly);
  d.put(p.rule_maxlen);
  d.put(p.rule_relax);
  d.put(p.rule_atoms);
  d.put(p.rule_winback);
  d.put(p.rule_prog);
  d.put(p.rule_rev);
  d.put(p.rule_fold_dfa);
  d.put(p.fold_all_dfa);
  d.put(p.fold_rules);
  d.put(p.allow_path_dfa);
  return d.h;
}
}  // namespace tsg
