/*
 * trivy_secret.h -- C ABI of the MI355X secret-scan engine (libtrivy_secret.so).
 *
 * Drop-in boundary for trivy's secret hot path, pkg/fanal/secret:
 *
 *   reference (Go)                                    this ABI
 *   ------------------------------------------------  ---------------------------------
 *   secret.NewScanner(*Config) Scanner                tsg_ruleset_compile
 *       scanner.go:293-329 (rule assembly stays in the host language; the final
 *       Global{Rules, AllowRules, ExcludeBlock} is handed over here)
 *   regexp compile error via Regexp.UnmarshalYAML     TSG_ERR_CONFIG + err text
 *       scanner.go:69-81
 *   Global.AllowPath(path) bool                       tsg_ruleset_allow_path
 *       scanner.go:55-57 (used by SecretAnalyzer.Required, analyzer/secret/secret.go:145)
 *   (*Scanner).Scan(ScanArgs) types.Secret            tsg_scan_cpu (one file, exact CPU)
 *       scanner.go:341-416                            tsg_scan_batch (many files, GPU)
 *                                                     tsg_scan_device (many files already
 *                                                       in this GPU's memory)
 *                                                     tsg_scan_device_spans (the same, as
 *                                                       spans of one device buffer)
 *   utils.IsBinary in SecretAnalyzer.Analyze          TSG_SPANS_BINARY_GATE (on the device)
 *       secret.go:78-84, utils.go:71-89
 *   SecretAnalyzer.Analyze per-file goroutines        tsg_queue_scan (concurrent callers
 *       analyzer/secret/secret.go:78-110,               coalesced into pinned batches),
 *       analyzer.go:419-443                             tsg_slot_* / tsg_scan_batch (batches)
 *   per-layer goroutines over a node's GPUs           tsg_multi_* (one process, N devices)
 *       artifact/image/image.go:210-234
 *
 * Error convention: every call returns TSG_OK (0) or a negative TSG_ERR_*; the
 * message of the last failing call on this thread is tsg_last_error().  No C++
 * exception crosses the ABI.  Every entry point is thread-safe (the GPU calls name the
 * caller's own slot and submission ticket; none acts on "the last" batch); a tsg_ruleset
 * is immutable and may be shared by any number of threads and contexts.  The library never
 * retains a caller pointer past a call, with one documented exception: the device buffer of
 * tsg_device_submit / tsg_device_spans_submit, which the caller leaves untouched until the
 * ticket is collected.
 *
 * Result format (tsg_result_data), little endian:
 *   u32 magic 'TSG1' (0x31475354), u32 nfiles, then per file:
 *     u8  status      0 = no findings  -> types.Secret{}             (scanner.go:401-403)
 *                     1 = path allowed -> types.Secret{FilePath}      (scanner.go:343-347)
 *                     2 = findings     -> types.Secret{FilePath, Findings}
 *     u32 nfindings, then per finding (already in Go sort.Slice order, scanner.go:405-410):
 *       u32 rule (index into the compiled rule list: RuleID/Category/Severity/Title)
 *       i32 start_line, i32 end_line, bytes match, u32 nlines, then per line:
 *         i32 number, u8 flags (1 IsCause, 2 FirstCause, 4 LastCause), bytes content
 *   bytes = u32 length + raw bytes (Content == Highlighted in the reference).
 */
#ifndef TRIVY_SECRET_H
#define TRIVY_SECRET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSG_OK 0
#define TSG_ERR_CONFIG -1  /* a regex failed to compile (Go regexp syntax) */
#define TSG_ERR_ARG -2     /* bad argument */
#define TSG_ERR_GPU -3     /* HIP runtime / device failure */
#define TSG_ERR_NOMEM -4   /* allocation failure */
#define TSG_ERR_INTERNAL -5

/* secret.AllowRule (scanner.go:186-191). NULL regex/path = field absent. */
typedef struct tsg_allow_rule_desc {
  const char* id;
  const char* description;
  const char* regex;
  const char* path;
} tsg_allow_rule_desc;

/* secret.Rule (scanner.go:83-94). NULL regex/path = field absent. */
typedef struct tsg_rule_desc {
  const char* id;
  const char* category;
  const char* title;
  const char* severity;
  const char* regex;
  const char* const* keywords;
  uint32_t n_keywords;
  const char* path;
  const tsg_allow_rule_desc* allow_rules;
  uint32_t n_allow_rules;
  const char* const* exclude_regexes; /* ExcludeBlock.Regexes */
  uint32_t n_exclude_regexes;
  const char* secret_group_name;
} tsg_rule_desc;

typedef struct tsg_ruleset tsg_ruleset;
typedef struct tsg_result tsg_result;
typedef struct tsg_ctx tsg_ctx;

/* Compile Global{Rules, AllowRules, ExcludeBlock}: regexes, the K1 keyword automaton,
 * the K2 rule-group DFAs.  On TSG_ERR_CONFIG, err holds Go's error text. */
int tsg_ruleset_compile(const tsg_rule_desc* rules, uint32_t n_rules,
                        const tsg_allow_rule_desc* allow_rules, uint32_t n_allow_rules,
                        const char* const* exclude_regexes, uint32_t n_exclude_regexes,
                        tsg_ruleset** out, char* err, size_t err_len);
void tsg_ruleset_destroy(tsg_ruleset* rs);

/* Global.AllowPath: 1 allowed, 0 not, <0 error. */
int tsg_ruleset_allow_path(const tsg_ruleset* rs, const char* path, size_t path_len);

typedef struct tsg_ruleset_info {
  uint32_t n_rules;
  uint32_t n_keywords;      /* K1 keyword ids incl. 3 fallback pseudo keywords */
  uint32_t n_groups;        /* K2 DFAs */
  uint32_t n_hostonly;      /* rules without a GPU DFA (state cap) */
  uint32_t kw_states;       /* K1 automaton states */
  uint32_t max_group_states;
  uint64_t table_bytes;     /* all device tables */
  uint32_t kw_classes;      /* K1 automaton byte classes */
  uint32_t k1x_literals;    /* literals of the hashed prefilter (K1X; large rule sets) */
} tsg_ruleset_info;
int tsg_ruleset_get_info(const tsg_ruleset* rs, tsg_ruleset_info* out);

/* Exact CPU Scan of one file (scanner.go:341-416). */
int tsg_scan_cpu(const tsg_ruleset* rs, const char* path, size_t path_len,
                 const uint8_t* content, size_t len, tsg_result** out);

/* Exact CPU Scan of a batch: file i = data[offsets[i] .. offsets[i+1]),
 * path i = paths[path_offsets[i] .. path_offsets[i+1]). nthreads <= 0: hardware. */
int tsg_scan_cpu_batch(const tsg_ruleset* rs, const uint8_t* data, const uint64_t* offsets,
                       uint32_t nfiles, const char* paths, const uint64_t* path_offsets,
                       int nthreads, tsg_result** out);

const uint8_t* tsg_result_data(const tsg_result* r, size_t* len);

/* sort.Slice with Go 1.19's pdqsort_func (unstable; ties ordered exactly as Go orders them)
 * of n items by (key bytes as a Go string, then secondary if not NULL): perm[k] = index of
 * the k-th item.  Replaces the secret part of AnalysisResult.Sort
 * (pkg/fanal/analyzer/analyzer.go:212-223): files by FilePath, findings by (RuleID,
 * StartLine). */
int tsg_go_sort_perm(const uint8_t* keys, const uint64_t* key_offsets, const int64_t* secondary,
                     uint32_t n, uint32_t* perm);
void tsg_result_free(tsg_result* r);
/* Counts of a result (bench and test checks): files, files with findings, findings. */
int tsg_result_summary(const tsg_result* r, uint64_t* nfiles, uint64_t* files_with_findings,
                       uint64_t* findings);

/* ---- GPU (one context per device) ----
 *
 * A context owns the rule tables on one device, two lanes (HIP stream + HBM buffers: the
 * H2D of one batch overlaps the kernels of the other), a pool of pinned host slots that
 * batches are staged in, and the host resolvers of batches in flight.  The library never
 * retains a caller pointer past a call (batch bytes are copied into, or written directly
 * by the caller into, library-owned pinned slots); the device-resident input below is the
 * exception and says so.
 *
 * Threading: every entry point below is thread-safe on a shared context.  No call acts on
 * "the last" anything: a caller names its own slot (slot id) and its own submission
 * (ticket), so concurrent per-layer / per-file callers (image.go:210-234,
 * analyzer.go:419-443) never see each other's batches. */
typedef struct tsg_ctx_options {
  uint32_t chunk_bytes;      /* bytes per lane (multiple of 16); 0 = default */
  uint32_t ext_cap;          /* max bytes a lane follows a match past its chunk; 0 = default */
  uint32_t cand_capacity;    /* candidate records per batch (K2 drops the records past it and
                                flags their files, which the host then resolves whole);
                                0 = 4 Mi */
  int32_t host_threads;      /* resolver threads; <= 0 = 16 */
  uint32_t adapt_mib;        /* first batch of at least this many MiB samples K1's literal
                                frequencies and stops reporting the frequent ones (their
                                keyword gates are then checked on the host); 0 = 16,
                                0xFFFFFFFF = never */
  uint32_t flags;            /* TSG_CTX_* */
  uint32_t slot_mib;         /* default capacity of a pinned slot (tsg_queue batches,
                                tsg_multi pieces); 0 = 256 */
  uint32_t max_slots;        /* pinned slots a context may hold; 0 = 16 */
} tsg_ctx_options;

/* Test mode: no HIP device is touched; the kernels' algorithm is emulated on the CPU over
 * the same slots, lanes and queue logic (tests of the pipeline and of tsg_queue on hosts
 * without a GPU).  Never chosen implicitly. */
#define TSG_CTX_EMULATE 1u

int tsg_ctx_create(int device, const tsg_ruleset* rs, const tsg_ctx_options* opt,
                   tsg_ctx** out);
/* Waits for every batch in flight, then frees the context. */
void tsg_ctx_destroy(tsg_ctx* ctx);

/* -- Zero-copy staging: the caller packs files straight into a pinned slot -------------
 * Replaces the per-file io.ReadAll copy of SecretAnalyzer.Analyze
 * (pkg/fanal/analyzer/secret/secret.go:85): ingest writes file bytes into the slot;
 * offsets[0] = path_offsets[0] = 0 and file i = data[offsets[i] .. offsets[i+1]),
 * path i = paths[path_offsets[i] .. path_offsets[i+1]). */
typedef struct tsg_slot_view {
  uint32_t id;
  uint8_t* data;            /* data_cap bytes */
  uint64_t data_cap;
  uint64_t* offsets;        /* files_cap + 1 */
  uint32_t files_cap;
  char* paths;              /* paths_cap bytes */
  uint64_t paths_cap;
  uint64_t* path_offsets;   /* files_cap + 1 */
} tsg_slot_view;
/* A free slot with at least these capacities (allocated or grown if needed), owned by the
 * caller until tsg_slot_release.  Waits while every slot is busy with submissions. */
int tsg_slot_acquire(tsg_ctx* ctx, uint64_t data_bytes, uint32_t nfiles, uint64_t path_bytes,
                     tsg_slot_view* out);
/* Submit the slot's first nfiles files: the device part runs asynchronously, the host
 * resolution follows it on the resolver pool.  *ticket names this submission for
 * tsg_batch_collect.  The slot may be submitted again (same bytes) at once, also with a
 * different nfiles: a submission reads the slot and never writes the bytes the caller can
 * reach (only a slot the library filled itself -- tsg_batch_upload -- submitted whole and
 * with nothing else in flight carries its zero tail and offsets in the room behind data_cap).
 * The slot must not be written until its submissions are collected. */
int tsg_slot_submit(tsg_ctx* ctx, uint32_t slot_id, uint32_t nfiles, uint64_t* ticket);
/* Give the slot back to the context (it is reused once its submissions are done). */
int tsg_slot_release(tsg_ctx* ctx, uint32_t slot_id);

/* -- Copying staging: the batch is copied into a free slot, which is then the caller's
 * (submit it with tsg_slot_submit, give it back with tsg_slot_release). */
int tsg_batch_upload(tsg_ctx* ctx, const uint8_t* data, const uint64_t* offsets,
                     uint32_t nfiles, const char* paths, const uint64_t* path_offsets,
                     uint32_t* slot_id);
/* Results of one submission (waits for its resolution); each ticket is collected once. */
int tsg_batch_collect(tsg_ctx* ctx, uint64_t ticket, tsg_result** out);
/* number of submitted, uncollected tickets of the context (all callers) */
int tsg_batch_pending(const tsg_ctx* ctx);
/* One batch, synchronously: copied into a slot of its own, scanned, resolved, slot freed
 * (the Scan of many files; thread-safe, any number of concurrent callers). */
int tsg_scan_batch(tsg_ctx* ctx, const uint8_t* data, const uint64_t* offsets, uint32_t nfiles,
                   const char* paths, const uint64_t* path_offsets, tsg_result** out);
/* Test hook: the device part of a scan of an acquired slot's first nfiles files,
 * synchronously, without resolution; writes K1's keyword bits [nfiles * kw_words] and chunk
 * event bits [ceil(bytes / chunk_bytes)] (either pointer may be NULL). */
int tsg_batch_kernels(tsg_ctx* ctx, uint32_t slot_id, uint32_t nfiles, uint32_t* kw,
                      size_t kw_len, uint32_t* ev, size_t ev_len);
/* Test hook: K2's work lists as the item passes of the last tsg_batch_kernels left them on
 * its lane (same slot, nothing submitted to the context in between: TSG_ERR_ARG otherwise;
 * synchronous, like tsg_batch_kernels).  n[0..2] = list entries, dense entries and the item
 * array in use on the device (tsg_stats.k2_items: a skipped list group keeps its region,
 * which may lie past the array's end and is not copied); up to the given capacities are
 * copied (any pointer may be NULL):
 *   entries   4 u32 each: {group, first item, items (<= 512, one group), 1}
 *   dentries  4 u32 each: {group, first chunk, chunks (<= 1,024), 2}
 *   items     2 u32 each: (file, chunk); a list group's items lie at [first item, + items)
 *             of its entries, in any order
 *   gskip     [n_groups] 1 = the group was skipped (left to the host) */
int tsg_batch_items(tsg_ctx* ctx, uint32_t slot_id, uint32_t* entries, size_t entries_cap,
                    uint32_t* dentries, size_t dentries_cap, uint32_t* items, size_t items_cap,
                    uint8_t* gskip, size_t gskip_len, uint64_t* n);
/* Test hook: what K2 and the outputs kernel of the last tsg_batch_kernels handed to the host,
 * read from the batch's pinned output block (same contract as tsg_batch_items: same slot,
 * nothing submitted in between, not on an emulated context: TSG_ERR_ARG otherwise).
 * n[0..3] = candidate records K2 reserved (tsg_stats.candidates), records in the block
 * (min(n[0], candidate capacity)), files of the batch, the candidate capacity; up to the
 * given capacities are copied (any pointer may be NULL):
 *   records  3 u32 each {file, rule, end}, as written, in the device's order (the forms:
 *            tsg_emulate_candidates)
 *   flags    [files] 1 = overflow (resolve the file whole), 2 = folding runes present,
 *            4 = the file's keyword row was written
 *   kw       [files * kw_words] the keyword rows of the files with flag 4, zero elsewhere */
int tsg_batch_candidates(tsg_ctx* ctx, uint32_t slot_id, uint32_t* records, size_t records_cap,
                         uint8_t* flags, size_t flags_len, uint32_t* kw, size_t kw_len, uint64_t* n);

/* Test hook: what the context's K1 adaptation decided (tsg_ctx_options.adapt_mib: once per
 * context, on the first batch of that size).  Read-only and synchronous, under the context
 * lock.  On an emulated context and before an adaptation it succeeds with adapted = 0. */
typedef struct tsg_adaptation_info {
  uint32_t adapted;      /* 1 once the sampling launch has run and its decision is applied */
  uint32_t k1_filter;    /* 1 = K1 is K1F, 0 = the automaton (or an emulated context) */
  uint32_t hot_states;   /* silenced ids: K1F literals, or accepting states of the automaton */
  uint32_t ev_hot;       /* OR of the silenced ids' event bits */
  uint64_t sample_bytes; /* bytes of the batch the sampling launch counted in */
  uint32_t n_keywords;   /* length of kw_unknown (tsg_ruleset_info.n_keywords) */
  uint32_t n_groups;     /* length of gate_open and event_everywhere */
  uint32_t n_literals;   /* length of hits and quiet: the K1 literals after a K1F adaptation,
                          * 0 otherwise (the automaton counts per state, not per literal) */
  uint32_t reserved;
} tsg_adaptation_info;
/* Up to the given lengths are copied (any array pointer may be NULL):
 *   kw_unknown        [n_keywords] 1 = K1 no longer reports the keyword: the vector the host
 *                     resolver gets (zeros before an adaptation)
 *   gate_open         [n_groups] 1 = every file passes the group's keyword gate ...
 *   event_everywhere  [n_groups] 1 = the group listens to every chunk: both as uploaded,
 *                     read back from the device's tables
 *   hits              [n_literals] the sampling launch's verified arrivals per K1 literal id
 *                     (tsg_ruleset_k1_literal), 0 for an id without a record in the filter
 *   quiet             [n_literals] 1 = the literal left the filter */
int tsg_test_adaptation(tsg_ctx* ctx, tsg_adaptation_info* info, uint8_t* kw_unknown,
                        size_t kw_unknown_len, uint8_t* gate_open, size_t gate_open_len,
                        uint8_t* event_everywhere, size_t event_everywhere_len, uint32_t* hits,
                        size_t hits_len, uint8_t* quiet, size_t quiet_len);

/* Test hook: the HBM buffers of the context's lanes.  A batch runs on one lane, in that lane's
 * buffers, which grow on demand and otherwise still hold the lane's previous batch; a test
 * that means to run a batch on used memory reads this before and after it.  Read-only and
 * synchronous, under the context lock; host values only (no device call); TSG_ERR_ARG on an
 * emulated context.  n[0..2] = lanes, buffers per lane, and the lane the last batch was
 * enqueued on (by any entry point; 0xFFFFFFFF before the first).  Up to bufs_cap records are
 * written (bufs may be NULL), lane by lane, each lane's buffers in the same order. */
typedef struct tsg_lane_buffer {
  char name[24];   /* the member's name in LaneState, NUL-terminated: "kw", "ev_bits", ... */
  uint64_t bytes;  /* capacity in bytes (0: never allocated) */
  uint64_t allocs; /* allocations so far: unchanged since an earlier call = same memory */
} tsg_lane_buffer;
int tsg_test_lane_buffers(tsg_ctx* ctx, tsg_lane_buffer* bufs, size_t bufs_cap, uint32_t* n);

/* Test hook: the layout of the automaton K1 (k1_kernel), which has two bodies.  Packed: rows
 * as 16-bit byte offsets, states x stride x 2 <= 65,536 bytes, a 128 KiB LDS image.  Legacy:
 * rows as entry indices, anything larger, a 156 KiB image with the class words replicated per
 * lane.  Host values only, no device call. */
typedef struct tsg_k1_layout {
  uint32_t packed;        /* 1 = packed, 0 = legacy */
  uint32_t states;        /* states of the keyword automaton (tsg_ruleset_info.kw_states) */
  uint32_t classes;       /* its byte classes (tsg_ruleset_info.kw_classes) */
  uint32_t stride;        /* u16 entries per row: the class count, padded to 2 mod 4 where that
                             neither changes the layout nor overflows the rows */
  uint32_t row_unit;      /* row of state id = id * row_unit (packed: stride * 2, bytes;
                             legacy: stride, entries) */
  uint32_t table_bytes;   /* the transition table as staged into LDS (whole dwords) */
  uint32_t lds_class;     /* legacy: LDS size class of the image, 0..2 (52, 80, 156 KiB) */
  uint32_t rep;           /* legacy: 1 = the class words are replicated per lane */
  uint32_t lds_kib;       /* the kernel's static LDS image, KiB */
  uint32_t threads;       /* its block size, 0 = no kernel is built for this layout */
  uint32_t blocks_per_cu; /* resident blocks per CU of its persistent grid */
  uint32_t kw_words;      /* tsg_test_k1_layout: 32-bit words of a keyword row */
  uint32_t k1_filter;     /* tsg_test_k1_layout: 1 = batches under 4 GiB run K1F instead */
  uint32_t reserved;
} tsg_k1_layout;
/* The layout an automaton of `states` x `classes` gets: pure arithmetic.  TSG_ERR_ARG where
 * device tables cannot be made of it: states = 0, classes = 0 or > 128, rows past 16 bits, a
 * table past LDS, or a layout no kernel is built for (out is filled all the same then). */
int tsg_test_k1_layout_of(uint32_t states, uint32_t classes, tsg_k1_layout* out);
/* The same record read from the context's device tables (they keep their layout through the
 * K1 adaptation), with kw_words and k1_filter.  Under the context lock; TSG_ERR_ARG on an
 * emulated context. */
int tsg_test_k1_layout(tsg_ctx* ctx, tsg_k1_layout* out);

typedef struct tsg_stats {
  double k1_ms;          /* K1 literal automaton + run counters, last collected batch (HIP events) */
  double k2_ms;          /* K2 rule-group DFAs (the persistent work-list launch) */
  double aux_ms;         /* the outputs kernel (results into pinned, host-mapped memory) */
  double resolve_ms;     /* host exact resolution (wall) */
  uint64_t bytes;        /* content bytes of the batch */
  uint64_t k2_bytes;     /* chunk bytes K2 scans (items listed x chunk) */
  uint64_t candidates;   /* candidate records produced */
  uint64_t files_resolved;  /* files with findings */
  uint32_t k2_launches;  /* K2 work-list entries */
  uint32_t overflow;     /* 1 if candidates > the context's cand_capacity (records dropped,
                            their files resolved whole) */
  double gate_ms;        /* keyword gates + items + device-side layout */
  uint64_t k2_items;     /* (file, chunk) items of K2's list groups (the item array in use: a
                            skipped list group's reserved region counts too) */
  uint32_t k1_hot_states;  /* K1 automaton states no longer reported (adaptation) */
  double h2d_ms;         /* H2D of the batch (pinned slot -> HBM) */
  uint32_t groups_skipped; /* rule groups K2 left to the host (item capacity) */
  uint64_t batches;      /* batches collected so far, and their sums: */
  uint64_t sum_bytes;
  double sum_k1_ms, sum_gate_ms, sum_k2_ms, sum_h2d_ms, sum_d2h_ms, sum_resolve_ms;
  double wait_ms;        /* last batch: its kernels waiting for the previous batch's */
  /* K2 diagnostics of the last batch (TSG_K2_DIAG=1 in the environment, else 0): bytes
   * followed past chunk ends, the longest such tail, tails over 4 KiB, words replayed for
   * accepts */
  uint32_t k2_tail_bytes, k2_tail_max, k2_long_tails, k2_replays;
  /* the rest of a batch's device work (HIP events on its lane): the prep kernel (zero fills,
   * coarse file map) and the H2D of the file offsets; aux_ms / sum_d2h_ms above are the
   * outputs kernel (results written into pinned, host-mapped memory) */
  double prep_ms, meta_ms, sum_prep_ms, sum_meta_ms;
  /* K1X (large rule sets) in the last batch: 16-B words listed with a prefilter hit, and
   * words verified inline because their block's list slice was full */
  uint32_t k1x_records, k1x_inline;
  /* K1F (the filter-and-verify K1) in the last batch: 16-B words listed with a filter hit,
   * and literal occurrences its verification confirmed */
  uint32_t k1f_listed, k1f_arrivals;
  /* chunks of the last batch whose K1 event word is not empty (the item passes' units) */
  uint32_t event_chunks;
  /* 1: K1 ran as the filter-and-verify K1F (k1f_kernel), 0: as the automaton (k1_kernel) */
  uint32_t k1_filter;
  /* last batch, by the device wall clock stamped inside the kernels: K1F's first block
   * start to its last block end; K1F's start to K2's last block end (every kernel and gap
   * of the chain); the gates pass's start to K2's end.  The first two are 0 when K1 was not
   * K1F (only K1F stamps its start); post_k1_clock_ms is set for both K1 variants */
  double k1_clock_ms, chain_clock_ms, post_k1_clock_ms;
  /* their sums over the batches collected so far */
  double sum_k1_clock_ms, sum_chain_clock_ms, sum_post_k1_clock_ms;
  /* last batch: entries of K2's dense pass (1,024 consecutive chunks each, per dense group) */
  uint32_t k2_dense_entries;
  /* 1: K2's list pass runs k2_kernel_rich on this device, 0: k2_kernel (the occupancy API
   * decides when the context is created) */
  uint32_t k2_rich;
  /* bytes of K1X's verify image (slot table, literal entries and bytes), 0 without K1X: up to
   * 128 KiB k1x_verify_kernel stages it in LDS, a larger one is read from global memory */
  uint32_t k1x_img_bytes;
} tsg_stats;
int tsg_ctx_get_stats(const tsg_ctx* ctx, tsg_stats* out);

/* -- Device-resident input: the batch's bytes already live in this device's HBM ---------
 * (a torch tensor, the output of a GPU decompressor).  d_data is a device pointer on the
 * context's device, at any byte alignment, covering offsets[nfiles] bytes that are written
 * when the call is made; offsets, paths and path_offsets are host arrays as for
 * tsg_scan_batch.  No content crosses PCIe in bulk: a kernel stages the bytes into the
 * lane's buffer (HBM -> HBM, one extra read and write of the batch), every scan kernel runs
 * unchanged, and after them only the files the host resolver reads (files with a candidate,
 * empty files, flagged files) are copied device -> host into a pinned slot that mirrors the
 * batch sparsely; when every file is needed (rules without a GPU program, a skipped rule
 * group) the whole batch is copied in one D2H instead.  The slot is as large as the batch.
 * The caller leaves d_data untouched until the ticket is collected (tsg_batch_collect);
 * tsg_scan_device is submit + collect.  Results are byte-identical to tsg_scan_batch's for
 * the same bytes on the same context.  TSG_ERR_ARG: NULL context, NULL d_data with a
 * non-empty batch, offsets that do not start at 0 or decrease.  Under TSG_CTX_EMULATE
 * d_data is an ordinary host pointer (nothing is staged; the fetch is a memcpy of the same
 * segments). */
int tsg_device_submit(tsg_ctx* ctx, const void* d_data, const uint64_t* offsets, uint32_t nfiles,
                      const char* paths, const uint64_t* path_offsets, uint64_t* ticket);
int tsg_scan_device(tsg_ctx* ctx, const void* d_data, const uint64_t* offsets, uint32_t nfiles,
                    const char* paths, const uint64_t* path_offsets, tsg_result** out);
typedef struct tsg_device_input_stats {
  /* last collected device-resident batch */
  double stage_ms;         /* the staging kernel (HIP events; also tsg_stats.h2d_ms); 0 emulated */
  double fetch_ms;         /* the fetch: kernel or D2H by HIP events (wall time when emulated) */
  uint64_t fetched_files;  /* files the host resolver reads (empty ones included) */
  uint64_t fetched_bytes;  /* their bytes: what crossed PCIe */
  /* all device-resident batches so far */
  uint64_t batches, sum_bytes, sum_fetched_bytes;
  double sum_stage_ms, sum_fetch_ms;
  uint32_t whole_batch_copy; /* last batch: 1 = every file was needed, one D2H of the batch */
} tsg_device_input_stats;
int tsg_ctx_get_device_input_stats(const tsg_ctx* ctx, tsg_device_input_stats* out);
/* Test hook: the pinned mirror of the last finished device-resident batch as its fetch left
 * it (TSG_ERR_ARG if there was none, or if its slot has been handed out again since: any
 * later batch may take it).  n[0] = the batch's
 * bytes, n[1] = fetched segments; up to data_cap mirror bytes and up to segs_cap segments
 * {offset, length} (2 u64 each, ascending, disjoint) are copied (either pointer may be
 * NULL). */
int tsg_test_device_mirror(tsg_ctx* ctx, uint8_t* data, uint64_t data_cap, uint64_t* segs,
                           size_t segs_cap, uint64_t* n);

/* -- Device-resident input, files as spans of one device buffer ------------------------
 * What a GPU decompressor leaves behind is a layer tar: file bodies at arbitrary offsets,
 * headers between them, binaries among them.  File i is the lengths[i] bytes at offset
 * starts[i] of the base_bytes bytes at d_base (a device pointer on the context's device, any
 * alignment; base_bytes may be far more than one batch holds: only the listed spans count).
 * Spans may come in any order, with gaps, and may overlap.  With TSG_SPANS_BINARY_GATE a
 * kernel applies utils.IsBinary (utils.go:71-89: a control byte in the first
 * min(length, 300) bytes) to every span and the binary files are dropped as
 * SecretAnalyzer.Analyze drops them (secret.go:78-84); the submitting thread waits for that
 * kernel (the only wait of the call), so kept[i] (1 = scanned, 0 = dropped; may be NULL) is
 * final when the call returns.  A kernel then gathers the kept spans back to back, in input
 * order, into the lane's buffer in the staging copy's place, every scan kernel runs
 * unchanged, and afterwards only the files the host resolver reads are gathered into the
 * batch's pinned slot (never the whole buffer).  The result holds one record per KEPT file,
 * in input order; no kept file is a valid, empty result.  The sum of the lengths obeys the
 * limits of tsg_device_submit's batch, and the slot is as large as that sum.  The caller
 * leaves the buffer untouched until the ticket is collected.  Results are byte-identical to
 * tsg_scan_batch's for the kept files' bytes.  TSG_ERR_ARG: NULL context or out pointer, a
 * span that is not inside [0, base_bytes) (start + length overflowing included), NULL d_base
 * with a non-empty span, unknown flag bits; the context keeps working after it.  Under
 * TSG_CTX_EMULATE d_base is a host pointer, the gate runs on the CPU and the gathers are
 * memcpy of the same segment lists.  These batches count in tsg_device_input_stats too
 * (stage_ms = the gather, whole_batch_copy = 0), the device_poison knob applies, and
 * tsg_test_device_mirror shows their mirror and segments in the kept files' back-to-back
 * coordinates. */
#define TSG_SPANS_BINARY_GATE 1u   /* drop files utils.IsBinary calls binary (device-side) */
int tsg_device_spans_submit(tsg_ctx* ctx, const void* d_base, uint64_t base_bytes,
                            const uint64_t* starts, const uint64_t* lengths, uint32_t nfiles,
                            const char* paths, const uint64_t* path_offsets, uint32_t flags,
                            uint8_t* kept, uint64_t* ticket);
int tsg_scan_device_spans(tsg_ctx* ctx, const void* d_base, uint64_t base_bytes,
                          const uint64_t* starts, const uint64_t* lengths, uint32_t nfiles,
                          const char* paths, const uint64_t* path_offsets, uint32_t flags,
                          uint8_t* kept, tsg_result** out);
typedef struct tsg_device_spans_stats {
  /* last finished spans batch */
  double gate_ms;        /* binary_gate_kernel by HIP events (wall time when emulated); 0 = gate off */
  double gather_ms;      /* the staging gather by HIP events (= tsg_device_input_stats.stage_ms); 0 emulated */
  double wait_ms;        /* wall time the submitting thread waited for the gate */
  uint64_t files_in, files_kept, files_dropped;
  uint64_t bytes_in, bytes_kept; /* sum of all lengths, of the kept files' lengths */
  /* all spans batches so far */
  uint64_t batches, sum_files_in, sum_files_kept, sum_files_dropped, sum_bytes_in, sum_bytes_kept;
  double sum_gate_ms, sum_gather_ms, sum_wait_ms;
} tsg_device_spans_stats;
int tsg_ctx_get_device_spans_stats(const tsg_ctx* ctx, tsg_device_spans_stats* out);

/* -- Submission queue for concurrent per-file callers ----------------------------------
 * The analyzer framework calls Analyze -> Scan from one goroutine per file
 * (pkg/fanal/analyzer/analyzer.go:419-443).  tsg_queue_scan is that Scan: any number of
 * threads call it at once; their files are packed into the open slot, a slot is submitted
 * when full or flush_us after its first file, and each call returns its own file's result
 * (tsg_result, one file, the format above) once its batch is resolved.  Files too large
 * for a slot are scanned by the exact CPU path (same results). */
typedef struct tsg_queue tsg_queue;
int tsg_queue_create(tsg_ctx* ctx, uint32_t flush_us, tsg_queue** out);
int tsg_queue_scan(tsg_queue* q, const char* path, size_t path_len, const uint8_t* content,
                   size_t len, tsg_result** out);
/* submit the open slot now */
int tsg_queue_flush(tsg_queue* q);
/* waits for every call in flight */
void tsg_queue_destroy(tsg_queue* q);

/* -- One process, several GPUs (multi.cpp) ------------------------------------------
 * trivy is one process: per-layer goroutines (pkg/fanal/artifact/image/image.go:210-234)
 * and per-file goroutines (pkg/fanal/analyzer/analyzer.go:419-443) drive every GPU of the
 * node from one address space.  tsg_multi holds one context per device (same options);
 * tsg_multi_scan_batch shards a batch's files over them, largest first onto the least
 * loaded device (LPT by bytes), copies each share straight into that device's pinned
 * slots (pieces of slot_mib), and returns the results in input order (tsg_result format),
 * identical to tsg_scan_batch on one context.  Thread-safe; no collective. */
typedef struct tsg_multi tsg_multi;
int tsg_multi_create(const int* devices, uint32_t n, const tsg_ruleset* rs,
                     const tsg_ctx_options* opt, tsg_multi** out);
int tsg_multi_size(const tsg_multi* m);
/* the i-th device's context (owned by m; e.g. for a tsg_queue per device) */
int tsg_multi_ctx(tsg_multi* m, uint32_t i, tsg_ctx** out);
int tsg_multi_scan_batch(tsg_multi* m, const uint8_t* data, const uint64_t* offsets,
                         uint32_t nfiles, const char* paths, const uint64_t* path_offsets,
                         tsg_result** out);
int tsg_multi_get_stats(const tsg_multi* m, uint32_t i, tsg_stats* out);
void tsg_multi_destroy(tsg_multi* m);

const char* tsg_last_error(void);

/* ---- test and measurement knobs ----
 * Process-wide switches that change how (never what) the library computes, for tests and
 * measurements only.  They are set through this call alone: the library reads no
 * environment variable that changes a plan, a kernel or a result (the profiling switches
 * TSG_PROF, TSG_PROF2, TSG_LAYER_PROF, TSG_K2_DIAG, TSG_K2_TRACE, TSG_K1F_TRACE and TSG_DEBUG_RESOLVE only
 * add timings, counters or traces).  value NULL or "" resets the knob.
 *   "tar_range_kib"   sub-range floor of the parallel tar index walk (default 64 MiB)
 *   "piece_mib"       piece floor of tsg_layer_scan / tsg_fs_scan (default 16)
 *   "pike_only"       "1": the Go-regexp matcher uses the Pike VM alone (no backtracker)
 *   "no_k1x"          "1": a rule set too large for K1's automaton is not split onto K1X
 *   "x_step"          1, 2 or 4: the K1X window step of the next plans (default: the widest
 *                     step whose K1 automaton fits the packed table)
 *   "emu_wordrec"     "1": emulated K2 writes one record per accepting 16-B word, as the
 *                     kernel does (tsg_scan_batch_emulated, TSG_CTX_EMULATE contexts)
 *   "emu_kw_unknown"  comma-separated keywords the emulated K1 leaves to the host, as
 *                     after its adaptation (tsg_scan_batch_emulated)
 *   "k1_automaton"    "1": contexts created next run K1 as the LDS automaton instead of the
 *                     filter-and-verify K1F (k1f.hpp)
 *   "group_states"    state cap of a K2 rule-group DFA in the next compiled rule sets
 *                     (default 2,048 for rule sets of up to 256 rules, else 1,024)
 *   "group_table_kib" table cap of a K2 rule-group DFA, 1..64 KiB (default 64 for rule
 *                     sets of up to 256 rules, else 48)
 *   "k1f_grid"        cap on K1F's blocks (default: one per CU): many tiles per wave in
 *                     small test batches
 *   "grid_cap"        N >= 1: at most N blocks in every launch whose grid comes from the
 *                     device or a constant (prep, stage, gather, fetch, binary gate, tar marks,
 *                     K1, K1F, K1X and its verification, the gates pass's compaction blocks,
 *                     both item passes, the three K2 kernels, outputs), so that a small test
 *                     batch takes each block through many rounds of its loop; read once per
 *                     batch or call; 0 (default): the grids as they are; negative: TSG_ERR_ARG
 *   "k1f_list"       "1": K1F lists the chunks with events itself (no gates pass; the item
 *                     passes gate files from their keyword bits)
 *   "k2_items_cap"    K2's item capacity in the next batches (default: twice the batch's
 *                     chunks, at least 65,536); list groups past it are left to the host
 *   "k2_max_dense"    1..16: rule groups the dense pass takes in the next batches (default
 *                     16); further groups that want it are left to the host
 *   "k2_no_word_recs" "1": K2 writes a record per accepting transition instead of one per
 *                     accepting 16-B word, as for rule sets of 16,384 groups and more (the
 *                     emulation then ignores emu_wordrec)
 *   "device_poison"   "1": tsg_device_submit / tsg_device_spans_submit fill the batch's pinned mirror, before the
 *                     fetch, with a repeating line that the builtin rules match (an AWS access
 *                     key id): a resolver read of a byte that was not fetched shows up as a
 *                     wrong finding
 * Returns TSG_ERR_ARG for an unknown name. */
int tsg_test_knob(const char* name, const char* value);

/* ---- test hooks: the Go-regexp engine and the DFA builder in isolation ---- */
typedef struct tsg_regex tsg_regex;
int tsg_regex_compile(const char* src, tsg_regex** out, char* err, size_t err_len);
void tsg_regex_free(tsg_regex* re);
int tsg_regex_num_slots(const tsg_regex* re);
/* regexp.MatchString: 1 / 0 */
int tsg_regex_match(const tsg_regex* re, const uint8_t* text, size_t len);
/* FindAllIndex (submatch=0, 2 slots/match) or FindAllSubmatchIndex (submatch=1).
 * Writes up to cap int64 values, returns the number of values needed (>= 0). */
int64_t tsg_regex_find_all(const tsg_regex* re, const uint8_t* text, size_t len, int submatch,
                           int64_t* out, size_t cap);
/* FindAll with a chosen matcher: 0 auto, 1 Pike VM only, 2 bit-state backtracker where
 * its visited table fits (results must not depend on the choice). */
int64_t tsg_regex_find_all_engine(const tsg_regex* re, const uint8_t* text, size_t len,
                                  int submatch, int engine, int64_t* out, size_t cap);
/* DFA candidate end offsets of one regex over text (all p where a match may end),
 * computed with the GPU lane algorithm (chunk bytes per lane). Returns count. */
int64_t tsg_regex_dfa_ends(const tsg_regex* re, const uint8_t* text, size_t len, uint32_t chunk,
                           int64_t* out, size_t cap);

/* Emulate K1+K2 on the CPU (no resolution) and report, per rule, the number of
 * candidate end offsets, and per rule group the bytes K2 scans (plan tuning). */
int tsg_emulate_candidate_stats(const tsg_ruleset* rs, const uint8_t* data,
                                const uint64_t* offsets, uint32_t nfiles, uint32_t chunk,
                                uint64_t* cand_per_rule, uint64_t* gated_bytes_per_group);

/* The item set K2 scans (plan.hpp emulate_items, which the emulation itself calls), from
 * k1_reference's output: group g, file f, chunk c is an item iff g is gated for f (always,
 * or one of its keywords' bits), c is a chunk of f (empty files have none) and a chunk in
 * [c, min(c + back_g, last chunk of f)] carries one of g's event bits; a group with back_g >
 * max_back listens to every chunk (16: the device's rule, 0xFFFFFFFF: the emulation's).
 * triples (or NULL): up to triples_cap sorted (group, file, chunk); counts (or NULL)
 * [n_groups]: items per group; *n_items (or NULL): all items. */
int tsg_emulate_items(const tsg_ruleset* rs, const uint8_t* data, const uint64_t* offsets,
                      uint32_t nfiles, uint32_t chunk, uint32_t max_back, uint32_t* triples,
                      size_t triples_cap, uint64_t* counts, uint64_t* n_items);

/* What K2 writes for one batch, record by record and in the device's own form (plan.hpp
 * emulate_candidates): the reference of tsg_batch_candidates.  chunk and ext_cap are the
 * context's chunk_bytes and ext_cap (the value in use, not 0), items_cap and max_dense the
 * layout's (tsg_layout_reference), word_recs = 0 the form of the k2_no_word_recs knob.  A
 * record is 3 u32 {file, rule, end}: rule < 2^31 is a rule index and end the match's end
 * offset in the file, the file's length for an accept at end of text, or 0xFFFFFFFF
 * ("resolve this rule over the whole file"); rule with bit 31 is a transition record {group
 * = bits 16-30, table index = bits 0-15} of the accepting transition at `end`; with bit 30
 * too (groups then have 14 bits) a word record: the row before the byte at `end`, whose
 * 16-byte word of the batch accepts.  No candidate capacity is applied.  records (or NULL):
 * up to records_cap records in reference order; *n_records (or NULL): all of them. */
int tsg_emulate_candidates(const tsg_ruleset* rs, const uint8_t* data, const uint64_t* offsets,
                           uint32_t nfiles, uint32_t chunk, uint32_t ext_cap, uint64_t items_cap,
                           uint32_t max_dense, uint32_t word_recs, uint32_t* records,
                           size_t records_cap, uint64_t* n_records);

/* The candidates of the emulation's own per-item form (plan.hpp emulate_kernels: run_segment
 * over every item of emulate_items(max_back = 16), a tail behind each, no layout and no
 * capacity), as (file, rule index, end) triples of 3 u32 in item order: the independent
 * restatement that tsg_emulate_candidates' unique triples must equal where no group is dense
 * and no tail reaches ext_cap.  triples (or NULL): up to triples_cap triples; *n_triples (or
 * NULL): all of them. */
int tsg_emulate_item_candidates(const tsg_ruleset* rs, const uint8_t* data, const uint64_t* offsets,
                                uint32_t nfiles, uint32_t chunk, uint32_t ext_cap, uint32_t* triples,
                                size_t triples_cap, uint64_t* n_triples);

/* K2 records -> candidates, as the host resolver expands them (plan.hpp expand_candidate):
 * triples of 3 u32 (file, rule index, end) in record order, 0xFFFFFFFF ends kept; a
 * transition record gives one triple per rule of its accept mask, a word record those of
 * every accepting transition from its byte to the end of its word (or file).  triples (or
 * NULL): up to triples_cap triples; *n_triples (or NULL): all of them. */
int tsg_expand_candidates(const tsg_ruleset* rs, const uint8_t* data, const uint64_t* offsets,
                          uint32_t nfiles, const uint32_t* records, size_t n_records,
                          uint32_t* triples, size_t triples_cap, uint64_t* n_triples);

/* The device's item layout restated on the host (plan.hpp layout_reference), groups in id
 * order: kind[g] = 0 no items, 1 list, 2 dense, 3 skipped.  A group with counts[g] * 2 >
 * nchunks wants the dense pass and gets it while fewer than max_dense groups before it wanted
 * it; any other group with items wants the region of the item array behind the regions of
 * the list-wanting groups before it (a skipped group keeps its region) and is listed when the
 * region ends within items_cap.  totals (or NULL) = {item array in use, list entries (512
 * items), dense entries (1,024 chunks), skipped groups}: tsg_stats' k2_items, k2_launches,
 * k2_dense_entries and groups_skipped. */
int tsg_layout_reference(const uint64_t* counts, uint32_t n_groups, uint64_t nchunks,
                         uint64_t items_cap, uint32_t max_dense, uint8_t* kind, uint64_t* totals);

/* K1 reference semantics on the CPU (plan.hpp k1_reference): same layout as
 * tsg_batch_k1_output. */
int tsg_emulate_k1(const tsg_ruleset* rs, const uint8_t* data, const uint64_t* offsets,
                   uint32_t nfiles, uint32_t chunk, uint32_t* kw, size_t kw_len, uint32_t* ev,
                   size_t ev_len);

/* K1F (the filter-and-verify K1, k1f.hpp) emulated on the CPU with the device's tables and
 * bit logic: keyword bits and chunk events in tsg_emulate_k1's layout; the literals listed
 * in quiet_ids are left out of the filter (the adaptation's hot literals), and with
 * sample_kib > 0 the filter is priced on the batch's first sample_kib KiB (as the
 * adaptation prices it on a sample of its batch).  stats (or NULL): {flagged word groups,
 * verified literal occurrences, records in the filter, 0}.  TSG_ERR_CONFIG when K1F does
 * not apply to the rule set (the automaton K1 runs then). */
int tsg_emulate_k1f(const tsg_ruleset* rs, const uint8_t* data, const uint64_t* offsets,
                    uint32_t nfiles, uint32_t chunk, const uint32_t* quiet_ids, uint32_t nquiet,
                    uint32_t sample_kib, uint32_t* kw, size_t kw_len, uint32_t* ev, size_t ev_len,
                    uint64_t* stats);

/* Plan introspection: per rule group id (-1 host-only), relaxation (-1 exact), max len. */
int tsg_ruleset_rule_plan(const tsg_ruleset* rs, uint32_t rule, int32_t* group, int32_t* relax,
                          int64_t* max_len);

/* Plan introspection: the rule's GPU program.  first_atom: the top-level atom the program
 * starts at (> 0: a suffix program, the atoms before it are left to the host); rule_atoms:
 * the top-level atoms it keeps from there (-1: all of them; >= 0: a prefix-cut program,
 * whose candidate end is the end of that prefix, at or before the match's end); winback: how
 * far before a candidate end the resolver lets a match start (-1: anywhere in the file);
 * has_rev: 1 when the resolver narrows a candidate with the reverse DFA of the whole regex
 * (never for a prefix-cut program: its candidates are no match ends).  A host-only rule
 * and a rule without a regex report first_atom 0, rule_atoms -1 and winback -1. */
int tsg_ruleset_rule_program(const tsg_ruleset* rs, uint32_t rule, int32_t* first_atom,
                             int32_t* rule_atoms, int64_t* winback, int32_t* has_rev);

/* Test hook: K2 group `group` of the plan.  nrules: its rule count (at most 64); rules: the
 * first min(nrules, cap) global rule indices in the group's local order (a rule's position is
 * its bit in the group DFA's accept masks); per_state: the accept layout of the group's
 * device table, from the decision the upload makes (dfa_layout.hpp) -- 1: every transition
 * out of a state has the same accepts, which are staged per state in LDS; 0: look-ahead, the
 * accepts differ per byte class (a trailing empty-width assertion) and are read per
 * transition.  Needs no device.  Any output pointer may be NULL; a group index past the plan
 * is TSG_ERR_ARG. */
int tsg_ruleset_group_table(const tsg_ruleset* rs, uint32_t group, uint32_t* nrules,
                            int32_t* per_state, uint32_t* rules, uint32_t cap);

/* Plan introspection: the rule's K1 event bits (1 run U, 2 run D, 4.. literal classes,
 * 1<<31 none), the largest distance from a GPU-program match start to its event byte,
 * and a description of the anchor. */
int tsg_ruleset_rule_anchor(const tsg_ruleset* rs, uint32_t rule, uint32_t* event, int64_t* evdist,
                            char* desc, size_t desc_len);

/* Plan introspection: K1 literal i (0 <= i < n; ids below tsg_ruleset_info.n_keywords are
 * keywords, the rest anchor literals): its bytes (min(len, cap) copied), length and event
 * bits.  TSG_ERR_ARG once i >= n. */
int tsg_ruleset_k1_literal(const tsg_ruleset* rs, uint32_t i, uint8_t* buf, uint32_t cap,
                           uint32_t* len, uint32_t* event);

/* Test hook: a 64-bit FNV-1a hash of a canonical serialisation of every member of the
 * compiled plan (K1 and K1X literals, every DFA's tables, every rule's program, anchor and
 * windows, the groups): two rule sets compiled to the same plan give the same digest, on any
 * number of CPUs. */
int tsg_ruleset_plan_digest(const tsg_ruleset* rs, uint64_t* out);

/* Emulate K1+K2 on the CPU with the GPU algorithm and resolve (tests). */
int tsg_scan_batch_emulated(const tsg_ruleset* rs, const uint8_t* data, const uint64_t* offsets,
                            uint32_t nfiles, const char* paths, const uint64_t* path_offsets,
                            uint32_t chunk, tsg_result** out);

/* Layer ingest, replaces walker.LayerTar.Walk (pkg/fanal/walker/tar.go:33-84)
 * + AnalyzerGroup.AnalyzeFile's Required gate (analyzer.go:399-409) + SecretAnalyzer.Required
 * (analyzer/secret/secret.go:112-150) + utils.IsBinary (utils.go:71-89): walks an uncompressed
 * layer tar held in memory and packs every file the secret analyzer would scan into one batch
 * (paths get the "/" prefix of image files, secret.go:90-96).  skip_files / skip_dirs are the
 * walker's --skip-files / --skip-dirs; config_path the secret config (Required skips its base
 * name).  A malformed archive is TSG_ERR_ARG ("failed to extract the archive", tar.go:40). */
typedef struct tsg_layer tsg_layer;
typedef struct tsg_layer_view {
  const uint8_t* data;           /* kept files back to back (tsg_batch_upload layout) */
  const uint64_t* offsets;       /* [nfiles + 1] */
  uint32_t nfiles;
  const uint8_t* paths;          /* scan paths back to back */
  const uint64_t* path_offsets;  /* [nfiles + 1] */
  const char* opq;               /* opaque dirs, each NUL-terminated (tar.go:48-51) */
  size_t opq_len;
  const char* wh;                /* whiteout files, each NUL-terminated (tar.go:53-57) */
  size_t wh_len;
  uint32_t walked;               /* regular files the walker handed to the analyzers */
} tsg_layer_view;
int tsg_layer_pack(const tsg_ruleset* rs, const uint8_t* tar, uint64_t tar_len,
                   const char* const* skip_files, uint32_t n_skip_files,
                   const char* const* skip_dirs, uint32_t n_skip_dirs, const char* config_path,
                   tsg_layer** out);
/* Rank `rank` of `world`'s share of the same layer (configs[2], one layer sharded across the
 * GPUs of a node): the header chain, whiteouts, opaque dirs and skip-dir logic are those of
 * the whole layer (every rank returns the same opq / wh / walked); the walked regular files
 * are cut into `world` contiguous runs of about equal bytes in archive order, and only this
 * rank's run is gated and packed.  The union over ranks equals tsg_layer_pack's batch. */
int tsg_layer_pack_shard(const tsg_ruleset* rs, const uint8_t* tar, uint64_t tar_len,
                         const char* const* skip_files, uint32_t n_skip_files,
                         const char* const* skip_dirs, uint32_t n_skip_dirs, const char* config_path,
                         uint32_t rank, uint32_t world, tsg_layer** out);
int tsg_layer_get(const tsg_layer* layer, tsg_layer_view* out);
/* The header index itself split over the ranks (configs[2] at N GPUs; replaces the whole-chain
 * walk of tar.go:33-84 that tsg_layer_pack_shard repeats on every rank).  Rank r owns the
 * entries whose header group starts in its 512-aligned byte range [lo, hi) of the tar.
 *   1. tsg_layer_range_walk: speculative walk of the range from its first block that
 *      checksums as a ustar header; info = {lo, hi, start, end} (start/end ~0: no header /
 *      malformed on the speculative chain).
 *   2. The ranks exchange info and fix the true chain in rank order: pos(0) = 0,
 *      pos(r+1) = the true end of range r, which is info.end when info.start == pos(r) (a
 *      walk from a group position is deterministic); otherwise rank r calls
 *      tsg_layer_range_sync(pos(r)) and publishes its end (trivy_amd/shard.py:layer_chain).
 *      Every rank calls tsg_layer_range_sync with its pos before steps 3-4.
 *   3. tsg_layer_range_dirs: the dirs this range adds to the walker's skipDirs (tar.go:62-66),
 *      NUL-terminated, in walk order; they are handed to the later ranks.
 *   4. tsg_layer_range_pack: tar.go:45-84 over the range's entries with the earlier ranks'
 *      skip dirs first, then Required / IsBinary and the pack.  opq / wh are the range's own.
 * The union over ranks equals tsg_layer_pack's batch; an archive error on the true chain is
 * returned by the sync of the range holding it, as one sequential walk would report it. */
typedef struct tsg_layer_range tsg_layer_range;
int tsg_layer_range_walk(const uint8_t* tar, uint64_t tar_len, uint32_t rank, uint32_t world,
                         tsg_layer_range** out, uint64_t info[4]);
int tsg_layer_range_sync(tsg_layer_range* range, uint64_t pos, uint64_t* end);
int tsg_layer_range_dirs(tsg_layer_range* range, const char* const* skip_dirs, uint32_t n_skip_dirs,
                         const char** out, uint64_t* out_len);
int tsg_layer_range_pack(const tsg_ruleset* rs, const tsg_layer_range* range,
                         const char* const* skip_files, uint32_t n_skip_files,
                         const char* const* skip_dirs, uint32_t n_skip_dirs,
                         const char* const* prior_dirs, uint32_t n_prior_dirs,
                         const char* config_path, tsg_layer** out);
void tsg_layer_range_free(tsg_layer_range* range);
/* Filesystem ingest (configs[0], trivy fs): replaces walker.FS.Walk (pkg/fanal/walker/fs.go:25-63)
 * + the fs artifact's relative paths (pkg/fanal/artifact/local/fs.go:83-100) + Required +
 * IsBinary; files are read in parallel and packed in path order (paths relative to root, no
 * "/" prefix).  Result in the same tsg_layer form (no whiteouts). */
int tsg_fs_pack(const tsg_ruleset* rs, const char* root, const char* const* skip_files,
                uint32_t n_skip_files, const char* const* skip_dirs, uint32_t n_skip_dirs,
                const char* config_path, tsg_layer** out);
/* One rank's share of a tree (configs[0] over several GPUs, one process each): every rank
 * lists the tree (no file opened), the listed files in path order are cut into `world`
 * contiguous runs of about equal bytes, and only this rank's run is read, IsBinary-gated
 * and packed.  Concatenated in rank order the shards are tsg_fs_pack's batch; walked is the
 * whole tree's. */
int tsg_fs_pack_shard(const tsg_ruleset* rs, const char* root, const char* const* skip_files,
                      uint32_t n_skip_files, const char* const* skip_dirs, uint32_t n_skip_dirs,
                      const char* config_path, uint32_t rank, uint32_t world, tsg_layer** out);
/* Ingest straight into a pinned slot: tsg_layer_pack / tsg_layer_range_pack /
 * tsg_fs_pack whose kept files are written into a slot acquired from ctx instead of pageable
 * memory, so no second copy precedes the upload: a layer's files are copied once, tar ->
 * slot, and a tree's files are read straight into it (pread).  The rule set is ctx's.  On
 * success *slot_id is the caller's, as after tsg_slot_acquire: the slot's offsets and paths
 * are filled in, so tsg_slot_submit(ctx, *slot_id, view.nfiles) scans it, and
 * tsg_slot_release gives it back; the tsg_layer's view (tsg_layer_get) points into the slot
 * and is valid until then.  Waits, like tsg_slot_acquire, while every slot is busy. */
int tsg_layer_pack_slot(tsg_ctx* ctx, const uint8_t* tar, uint64_t tar_len,
                        const char* const* skip_files, uint32_t n_skip_files,
                        const char* const* skip_dirs, uint32_t n_skip_dirs, const char* config_path,
                        uint32_t* slot_id, tsg_layer** out);
int tsg_layer_range_pack_slot(tsg_ctx* ctx, const tsg_layer_range* range,
                              const char* const* skip_files, uint32_t n_skip_files,
                              const char* const* skip_dirs, uint32_t n_skip_dirs,
                              const char* const* prior_dirs, uint32_t n_prior_dirs,
                              const char* config_path, uint32_t* slot_id, tsg_layer** out);
int tsg_fs_pack_slot(tsg_ctx* ctx, const char* root, const char* const* skip_files,
                     uint32_t n_skip_files, const char* const* skip_dirs, uint32_t n_skip_dirs,
                     const char* config_path, uint32_t* slot_id, tsg_layer** out);
/* One call per layer / tree, pipelined (what a per-layer goroutine binds,
 * pkg/fanal/artifact/image/image.go:210-234): the walk and gates of tsg_layer_pack /
 * tsg_fs_pack, then the kept files cut in walk order into pieces of about the context's slot
 * size; each piece is written straight into a pinned slot and submitted while the next one
 * is written, so ingest, upload, kernels and host resolution overlap.  *out holds one record
 * per kept file in the order of *layer's paths (tsg_result format); *layer carries the paths,
 * offsets, opq, wh and walked count (its data view is NULL: the bytes lived in the slots).
 * tsg_fs_scan opens no file during its walk: every file that passes Required is listed with
 * its lstat size and read straight into its place in a piece; a file that is binary
 * (IsBinary on the bytes read) or cannot be opened is scanned along and then left out of
 * *out and *layer, which therefore equal tsg_fs_pack's batch and its scan. */
int tsg_layer_scan(tsg_ctx* ctx, const uint8_t* tar, uint64_t tar_len,
                   const char* const* skip_files, uint32_t n_skip_files,
                   const char* const* skip_dirs, uint32_t n_skip_dirs, const char* config_path,
                   tsg_layer** layer, tsg_result** out);
int tsg_fs_scan(tsg_ctx* ctx, const char* root, const char* const* skip_files, uint32_t n_skip_files,
                const char* const* skip_dirs, uint32_t n_skip_dirs, const char* config_path,
                tsg_layer** layer, tsg_result** out);
void tsg_layer_free(tsg_layer* layer);

/* -- Device-resident input, a whole layer tar ------------------------------------------
 * tsg_layer_scan for an uncompressed layer tar that lies in this GPU's memory (what a GPU
 * decompressor leaves behind): d_tar is a device pointer on the context's device, any
 * alignment, tar_len bytes.  One kernel (tar_mark_kernel) reads the tar once and marks, per
 * 512-byte block, whether it passes archive/tar's header checksum and whether it is all
 * zero; the two bitmaps come back in one copy.  Every marked block (512 bytes each) is
 * gathered into pinned memory, and archive/tar's Reader.Next walks the header chain on the
 * host over that sparse view: a position whose block is marked is read from the gathered
 * copy, an all-zero block is a zero block, anything else is "invalid header" -- what the
 * checksum test gives on the full bytes.  Blocks inside a member's data that happen to
 * checksum (a tar stored in the tar) are fetched and never reached.  The payloads of PAX 'x'
 * and GNU 'L' / 'K' headers are gathered in rounds: the chain is walked with the headers'
 * own sizes, the extended headers met are fetched in one launch, and the walk is repeated
 * until it needed nothing it did not have (an ordinary tar: one round, or none).  The
 * walker's whiteout / skip logic and SecretAnalyzer.Required then run on the host as in
 * tsg_layer_scan; the kept entries go, in walk order and in batches cut like
 * tsg_layer_scan's pieces, through tsg_device_spans_submit with TSG_SPANS_BINARY_GATE,
 * several batches in flight.  So only the header blocks, the extended-header payloads, the
 * bitmaps (2 bits per block) and the files the resolver reads cross PCIe.
 * *layer and *out are what tsg_layer_scan returns for the same bytes in host memory, field
 * for field (the layer's data view is NULL: the files are not packed on the host); a
 * malformed archive fails with TSG_ERR_ARG and the same "failed to extract the archive: ..."
 * text.  TSG_ERR_ARG too: NULL ctx, layer or out; NULL d_tar with tar_len > 0.  The context
 * keeps working after an error.  Thread-safe against other submitters on the context; the
 * caller leaves the buffer untouched until the call returns.  Under TSG_CTX_EMULATE d_tar is
 * a host pointer, the marks are a CPU loop and the gathers memcpy of the same lists. */
int tsg_device_layer_scan(tsg_ctx* ctx, const void* d_tar, uint64_t tar_len,
                          const char* const* skip_files, uint32_t n_skip_files,
                          const char* const* skip_dirs, uint32_t n_skip_dirs,
                          const char* config_path, tsg_layer** layer, tsg_result** out);
typedef struct tsg_device_layer_stats {
  /* last successful tsg_device_layer_scan */
  double mark_ms;            /* tar_mark_kernel by HIP events (wall time when emulated) */
  uint64_t tar_bytes;
  uint64_t blocks;           /* whole 512-byte blocks of the tar */
  uint64_t marked_blocks;    /* blocks that pass the header checksum */
  uint64_t chain_entries;    /* members on the header chain (after extended headers are applied) */
  uint64_t header_bytes;     /* header blocks fetched: 512 * marked_blocks */
  uint64_t payloads;         /* extended-header payloads fetched */
  uint64_t payload_bytes;
  uint64_t payload_rounds;   /* gather launches for them */
  uint64_t span_batches;     /* tsg_device_spans_submit batches */
  uint64_t files_scanned;    /* files in the result (Required and not binary) */
  uint64_t fetched_bytes;    /* files the batches' resolvers read (tsg_device_input_stats.fetched_bytes) */
  uint64_t pcie_bytes;       /* header_bytes + payload_bytes + fetched_bytes */
  /* all successful calls so far */
  uint64_t calls, sum_tar_bytes, sum_blocks, sum_marked_blocks, sum_chain_entries, sum_header_bytes,
      sum_payloads, sum_payload_bytes, sum_payload_rounds, sum_span_batches, sum_files_scanned,
      sum_fetched_bytes, sum_pcie_bytes;
  double sum_mark_ms;
} tsg_device_layer_stats;
int tsg_ctx_get_device_layer_stats(const tsg_ctx* ctx, tsg_device_layer_stats* out);
/* Test hook: the two bitmaps as tar_mark_kernel (or its emulation) leaves them for the
 * tar_len bytes at d_tar: bit b % 64 of word b / 64 belongs to block b, (tar_len / 512 + 63)
 * / 64 words each; words_cap is the room of both arrays (TSG_ERR_ARG if it is too small). */
int tsg_test_device_tar_marks(tsg_ctx* ctx, const void* d_tar, uint64_t tar_len,
                              uint64_t* header_bits, uint64_t* zero_bits, uint64_t words_cap);

#ifdef __cplusplus
}
#endif
#endif /* TRIVY_SECRET_H */
