/*
 * include/caps_sa_hip.h -- C ABI of the MI355X suffix-array / LCP-array construction path.
 *
 * This is the drop-in boundary: a plain-C shared library (libcaps_sa_hip.so) that sits
 * UNDER the reference's class surface CaPS_SA::Suffix_Array<idx> (reference
 * include/Suffix_Array.hpp:148-181).  The reference has no FFI of its own -- its only
 * caller is src/main.cpp:78-80,84-86 -- so each entry point cites the C++ member it
 * replaces.  caps-sa_amd/csrc/Suffix_Array.hpp is the host-side mirror of that class
 * whose construct() calls caps_sa_hip_build_u32/_u64; INTEGRATION.md shows the binding a
 * reference maintainer would add.
 *
 * Conventions: no exceptions, no exit(): every function returns 0 on success or a
 * negative CAPS_SA_E* code (the reference calls std::exit, src/Suffix_Array.cpp:33-37);
 * caps_sa_hip_last_error() returns a thread-local message.  Index width is chosen by
 * the caller exactly like src/main.cpp:76-87 (n <= UINT32_MAX -> _u32, else _u64).
 * Output is THE suffix array and LCP array of T[0..n): shorter suffix first when one is
 * a prefix of the other, bytes ordered as signed char (src/Suffix_Array.cpp:75-77),
 * LCP[0] = 0.  It does not depend on subproblem_count.
 */
#ifndef CAPS_SA_HIP_H
#define CAPS_SA_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CAPS_SA_OK 0
#define CAPS_SA_EINVAL (-1)       /* bad argument (null pointer, n too large for the index type) */
#define CAPS_SA_EUNSUPPORTED (-2) /* bounded max_context on several devices / in a shard, or with fewer than two subproblems */
#define CAPS_SA_EHIP (-3)         /* HIP runtime error; see caps_sa_hip_last_error() */
#define CAPS_SA_ENOMEM (-4)       /* device or host allocation failed */
#define CAPS_SA_ENODEVICE (-5)    /* no usable GPU */
#define CAPS_SA_EALPHABET (-6)    /* the workspace was sized for a 2-bit text (caps_sa_hip_workspace_bytes_ex), the text has more than 4 bytes;
                                     caps_sa_hip_fm_build_*: the BWT has more than 4 distinct bytes
                                     (caps_sa_hip_fm_build_wide_* takes 1 .. 256) */

/* Per-build record; replaces the per-phase stderr lines of construct()
 * (src/Suffix_Array.cpp:469-493).  Times are HIP-event milliseconds on the build's stream. */
typedef struct caps_sa_stats {
    uint64_t n;
    uint32_t idx_bytes;            /* 4 or 8 */
    uint32_t p_eff;                /* effective subproblem count, src/Suffix_Array.cpp:24 */
    uint32_t ppp;                  /* samples per subarray, src/Suffix_Array.cpp:27 */
    uint32_t bits_per_char;        /* 2 (alphabet <= 4 symbols) or 8 */
    uint32_t merge_passes_phase1, merge_passes_phase2, merge_passes_samples;
    uint32_t long_runs;            /* 1: the text holds a periodic stretch (period <= 16 chars) of >= 1024 chars and the
                                      comparators skipped such stretches through the run table (csrc/text.h) */
    uint64_t max_partition;        /* largest partition (elements) */
    uint64_t workspace_bytes;
    double ms_total;               /* whole build, device-resident interval */
    double ms_pack;                /* alphabet scan + text packing */
    double ms_sort_subarrays;      /* a5  sort_subarrays        (cpp:161-184) */
    double ms_select_pivots;       /* a6  select_pivots         (cpp:197-222) */
    double ms_locate_pivots;       /* a8  locate_pivots         (cpp:225-249) */
    double ms_partition;           /* a9  partition_sub_subarrays (cpp:300-368) */
    double ms_merge_partitions;    /* a10 merge_sub_subarrays   (cpp:371-409) */
    double ms_boundary_lcp;        /* a11 compute_partition_boundary_lcp (cpp:431-447) */
    double ms_output;              /* copy of SA/LCP into the caller's device buffers */
    double ms_h2d, ms_d2h;         /* host-buffer entry points only */
    /* the two tile-granular kernels, summed over their launches in this build */
    double merge_pass_ms;  uint64_t merge_pass_launches;  uint64_t merge_pass_elems;
    double tile_sort_ms;   uint64_t tile_sort_launches;   uint64_t tile_sort_elems;
    /* bucketing (count + scatter kernels) and collate, same convention */
    double bucket_scatter_ms; uint64_t bucket_scatter_launches; uint64_t bucket_scatter_elems;
    double bucket_count_ms;
    double collate_ms;
    /* bucket splits done without a count pass (fixed-capacity slots) / splits that had to be redone with one */
    uint32_t slot_splits, slot_splits_redone;
    /* Which construction ran.  1 = direct path: pivots sampled from the text, ONE scatter of the text into groups of
     * partitions, then the per-partition sort (select_pivots -> partition -> merge_partitions; sort_subarrays and
     * locate_pivots are skipped: their order would be discarded).  0 = samplesort path, all six phases of construct().
     * path_fallback: why a build that tried the direct path took the samplesort path after all (CAPS_SA_FB_*). */
    uint32_t path_direct, path_fallback;
    uint32_t direct_groups;        /* groups of consecutive partitions the text was scattered into */
    uint32_t direct_quantile;      /* 1: level B's buckets were sample quantiles (skewed keys / frequent keys), 0: linear maps */
    uint64_t direct_max_group;     /* largest stream of a group (elements) */
    double level_a_ms;             /* direct path: the text -> groups scatter (also counted in bucket_scatter_ms) */
    uint32_t direct_key_bits;      /* key bits that travelled with every suffix through the direct path's passes: 64, or 32 */
    uint32_t run_buckets;          /* buckets of ONE single-letter key (the suffixes deep inside N-blocks) that were ordered by
                                      (terminator class, rest of the run, text behind it) instead of being compared: csrc/text.h */
    uint32_t result_waves;         /* host-buffer entry points: slices in which SA / LCP left the device while later groups were still
                                      being sorted (1: one copy after the build) */
    uint32_t n_devices;            /* caps_sa_hip_build_multi_*: devices that built (1 elsewhere) */
    /* caps_sa_hip_build_multi_*: host wall clock of the three stages, the slowest and the fastest device of each (ms) */
    double ms_upload_max, ms_upload_min;       /* text to the device: ONE chunked upload to the first device, fanned out to the others
                                                  over xGMI chunk by chunk; a device's figure ends when its last chunk has arrived, so
                                                  it includes the wait for the devices served before it */
    double ms_device_build_max, ms_device_build_min;   /* level A .. boundary LCPs of the device's slice */
    double ms_download_max, ms_download_min;   /* the device's slice of SA / LCP to the caller's arrays */
    /* Groups of suffixes with one and the same key (64 / bits_per_char chars) that the sort did not settle by comparison but by
     * re-keying them deeper, level by level, afterwards (csrc/kernels.h "Deferred ties": tandem arrays, repeat families), their
     * members, and the deepest level (each 64 / bits_per_char chars). */
    uint64_t tie_groups_deferred, tie_elems_deferred;
    uint32_t tie_levels;
    uint32_t lcp_bytes_on_link;    /* host-buffer entry points: bytes per LCP value on the PCIe link -- 1 when the values left the device as
                                      bytes (+ a list of the values of 255 and more) and were widened on the host, else the index width */
    /* the three parts of the last stage, summed over their launches (device time, as the kernel clocks above): gathering SA / LCP
     * with the segment-head LCPs (a11), the letter-run buckets (run_buckets), the deferred ties (tie_groups_deferred) */
    double finish_ms, run_bucket_ms, msd_ms;
    /* direct path, quantile mode: level-B splits by knots done WITHOUT the count pass (slots + a stream for what outgrows them) /
     * redone with it (the stream ran full), and the elements that took the stream */
    uint32_t knot_slot_splits, knot_slot_splits_redone;
    uint64_t spill_entries;
    /* direct path: which hand-overs between its passes travelled as 12-byte (64-bit key, 32-bit index) records instead of a key
     * array and an index array -- a mask, bit 0 = level A -> level B (the only hand-over built so; the other bits are 0).  The environment
     * variable CAPS_SA_RECORDS chooses, 0 = none; always 0 with 64-bit indices, with 32-bit keys, and for a build that did not take
     * the direct path */
    uint32_t direct_records;
    /* direct path: the stages of the shortened start of a tile that the final sort's tile_sort_kernel launch ran with -- a mask, bit 0 =
     * the bucket-indexed launch (workgroup g sorts bucket g and loads its slot before anything else; csrc/kernels.h).  The environment
     * variable CAPS_SA_TILE_CHAIN chooses, 0 = the launch over the tile table; always 0 in quantile mode, with 64-bit indices, with
     * 32-bit keys, when a slot overflowed and the split was redone, for a build that leaves in waves, and off the direct path */
    uint32_t tile_chain;
    /* direct path: which scatter kernels issued a tile's memory traffic together (csrc/kernels.h ISSUE) -- a mask, bit 0 = level B
     * (all loads of a tile ahead of its bucket map, the emit's stores back to back; the only stage built so, the other bits are 0).
     * The environment variable CAPS_SA_SCATTER_ISSUE chooses, 0 = the plain kernels; always 0 in quantile mode, with
     * 64-bit indices, with 32-bit keys, without records, for a build that leaves in waves, and off the direct path */
    uint32_t scatter_issue;
    /* direct path: what level B handed to the final sort in its slots -- a mask, bit 0 = 8-byte records of a bucket-relative 32-bit key
     * and the index instead of a 64-bit key array and an index array (csrc/kernels.h "slot keys"; the only stage built so, the other
     * bits are 0).  The environment variable CAPS_SA_SLOT_KEYS chooses, 0 = the two arrays; always 0 where tile_chain or scatter_issue
     * is 0, on 8-bit texts, when a slot overflowed and the split was redone, and off the direct path */
    uint32_t slot_keys;
} caps_sa_stats;

/* sizeof(caps_sa_stats) / sizeof(caps_sa_shard_info) of THIS library.  Both structs grow at their end from release to release and
 * the entry points write all of them: a caller compiled against an older header must check these against its own sizeof before
 * passing a buffer (caps-sa_amd/_binding.py does at load time). */
uint32_t caps_sa_hip_stats_bytes(void);
uint32_t caps_sa_hip_shard_info_bytes(void);

#define CAPS_SA_FB_NONE 0
#define CAPS_SA_FB_FORCED 1        /* CAPS_SA_PATH=classic */
#define CAPS_SA_FB_SHAPE 2         /* too small / too few subproblems for a two-level distribution */
#define CAPS_SA_FB_LONG_RUNS 3     /* the text holds a long periodic stretch: keys alone cannot split it */
#define CAPS_SA_FB_PIVOT_TIES 4    /* two sampled pivots share their key */
#define CAPS_SA_FB_GROUP_OVERFLOW 5 /* a group outgrew its region (a very frequent key) */
#define CAPS_SA_FB_KEY32 6         /* sharded build: a bucket slot overflowed under 32-bit keys; repeat with caps_sa_hip_shard_set_key_bits(s, 64) */
#define CAPS_SA_FB_BOUNDED 7       /* 0 < max_context < n: the reference's own sequence, one thread per merge node (csrc/bounded.h) */

int caps_sa_hip_device_count(void);
const char* caps_sa_hip_last_error(void);
const char* caps_sa_hip_version(void);

/*
 * The host-buffer entry points (caps_sa_hip_build_*) keep their device memory (text, SA, LCP,
 * workspace) between calls -- allocating and freeing tens of GB costs far more than a build.
 * One grow-only block per process; this releases it.  (The reference frees everything in
 * clean_up() / the destructor, src/Suffix_Array.cpp:42-45,455-459; a caller that wants that
 * behaviour calls this after construct().)
 */
void caps_sa_hip_release_cache(void);

/*
 * Page-locked host memory for SA / LCP buffers (the reference mallocs them in its constructor,
 * src/Suffix_Array.cpp:20-21).  Results land in such buffers at the PCIe link rate; pageable
 * buffers work too, slower.  Returns NULL on failure (caps_sa_hip_last_error()).
 */
void* caps_sa_hip_host_alloc(uint64_t bytes);
void caps_sa_hip_host_free(void* p);

/*
 * The reference's input generator, utils/gen_rand_seq.py:9-13 -- random.seed(seed); n x random.choice(['A','C','G','T']) --
 * bit for bit: MT19937 seeded like CPython's random.seed(int) (init_by_array([seed])), every choice = the top 3 bits of one
 * 32-bit output, drawn again while >= 4 (random.choice -> _randbelow(4) -> getrandbits(3)).  Writes n letters to out (host
 * memory; the script's print() adds a newline, which the CLI remaps to 'C': callers append it themselves).  Host code, no
 * GPU: ~5 ns per letter.  BASELINE's workloads are quoted on this stream, so bench.py builds C2 / C3 from it.
 */
int caps_sa_hip_gen_rand_seq(uint32_t seed, uint64_t n, char* out);

/* Device workspace a build of n suffixes needs (bytes), for any text. */
int caps_sa_hip_workspace_bytes(uint64_t n, uint64_t subproblem_count, int idx_bytes, uint64_t* bytes);
/* The same for a text of at most 4 distinct bytes (bits_per_char = 2: everything behind the reference CLI, src/main.cpp:61-70):
 * the packed text and its run table then take n / 2 bytes instead of 2 n.  caps_sa_hip_build_device_* reads the alphabet it
 * may assume off the size of the workspace it is given; a text with more letters is refused with CAPS_SA_EALPHABET.
 * bits_per_char = 8 is caps_sa_hip_workspace_bytes. */
int caps_sa_hip_workspace_bytes_ex(uint64_t n, uint64_t subproblem_count, int idx_bytes, int bits_per_char, uint64_t* bytes);

/*
 * Replaces the body of Suffix_Array<uint32_t>::construct() / <uint64_t>
 * (src/Suffix_Array.cpp:466-494; constructor arguments of include/Suffix_Array.hpp:155).
 * T: n bytes, host memory, borrowed.  SA, LCP: n entries each, host memory owned by the
 * caller (the class allocates them in its constructor, src/Suffix_Array.cpp:20-21).
 * subproblem_count 0 -> 8192 (include/Suffix_Array.hpp:42), clamped to n/16 (cpp:24).
 * max_context 0 or >= n: THE suffix array and LCP array of T.  0 < max_context < n: the reference's bounded-context result
 * (comparisons stop after max_context chars, ties keep the reference's merge history: csrc/bounded.h; parity unpinned by any
 * reference-held vector, a compatibility mode that is seconds, not milliseconds).  device: HIP device ordinal.
 */
int caps_sa_hip_build_u32(const char* T, uint64_t n, uint64_t subproblem_count, uint64_t max_context,
                          uint32_t* SA, uint32_t* LCP, int device, caps_sa_stats* stats);
int caps_sa_hip_build_u64(const char* T, uint64_t n, uint64_t subproblem_count, uint64_t max_context,
                          uint64_t* SA, uint64_t* LCP, int device, caps_sa_stats* stats);

/*
 * construct() on several GPUs of one node from ONE process (what Suffix_Array(T, n, p, ctx, devices)
 * calls): devices[0 .. n_devices) are HIP device ordinals, one rank of the sharded direct path each (a device may be listed
 * more than once).  The text is copied to every device.  Default: NO element crosses a link -- every device classifies the
 * whole text (level A), keeps the suffixes of the groups of partitions it owns (1 / n_devices of them), sorts them and
 * copies its slice of SA / LCP into the caller's arrays; per device: the packed text + about 2.7 x 16 B x n / n_devices of
 * work arrays.  CAPS_SA_SHARD_EXCHANGE=1 selects the variant in which every device classifies every n_devices-th tile only
 * and the blocks of (key, sa) are then copied device to device over xGMI (8.8 B per suffix).  n_devices = 1 is
 * caps_sa_hip_build_*.  Texts the direct path does not
 * take (stats->path_fallback says why) are built on devices[0] alone.  stats: host wall-clock per stage, all devices.
 */
int caps_sa_hip_build_multi_u32(const char* T, uint64_t n, uint64_t subproblem_count, uint64_t max_context,
                                uint32_t* SA, uint32_t* LCP, const int* devices, int n_devices, caps_sa_stats* stats);
int caps_sa_hip_build_multi_u64(const char* T, uint64_t n, uint64_t subproblem_count, uint64_t max_context,
                                uint64_t* SA, uint64_t* LCP, const int* devices, int n_devices, caps_sa_stats* stats);

/*
 * Same construction with everything resident in HBM: dT (n bytes), dSA, dLCP (n entries)
 * are device pointers on the current device; hip_stream is a hipStream_t (NULL = default
 * stream).  workspace: device memory of at least caps_sa_hip_workspace_bytes(), or NULL
 * to let the call allocate and free it.  Returns after the stream work has completed.
 */
int caps_sa_hip_build_device_u32(const void* dT, uint64_t n, uint64_t subproblem_count, uint64_t max_context,
                                 void* dSA, void* dLCP, void* workspace, uint64_t workspace_bytes,
                                 void* hip_stream, caps_sa_stats* stats);
int caps_sa_hip_build_device_u64(const void* dT, uint64_t n, uint64_t subproblem_count, uint64_t max_context,
                                 void* dSA, void* dLCP, void* workspace, uint64_t workspace_bytes,
                                 void* hip_stream, caps_sa_stats* stats);

/*
 * Device verifier in the spirit of the reference's (never called) is_sorted
 * (src/Suffix_Array.cpp:512-536) plus a permutation check; byte loops on the raw text,
 * independent of the build kernels' packed text.  *n_errors = 0 iff (dSA, dLCP) is the
 * suffix array and LCP array of dT.
 *
 * What *n_errors counts (cnt = n and is_head = 1 here; the slice calls below pass their own).  Per entry i < cnt:
 *   - SA[i] >= n counts 1, and nothing else is counted for that entry.
 *   - Otherwise:
 *       - a value already met in this call counts 1 (k copies of a value give k - 1);
 *       - i == 0: counts 1 if is_head is set and LCP[0] != 0;
 *       - i > 0 with SA[i-1] < n: counts 1 if LCP[i] is not the exact common prefix of the suffixes SA[i-1] and SA[i];
 *       - i > 0 with SA[i-1] < n: counts 1 more if the pair is not in strictly increasing order.  The order is on signed
 *         bytes, with a proper prefix first: the longer suffix before its own proper prefix is the violation (a value next
 *         to itself is a repeat, not an order error).
 *     A pair whose left entry SA[i-1] >= n is not looked at: that entry has been counted on its own.
 * n == 0 or cnt == 0: CAPS_SA_OK with *n_errors = 0, whatever the pointers.  cnt > n, a null n_errors, or a null dT / dSA /
 * dLCP with something to check: CAPS_SA_EINVAL.
 */
int caps_sa_hip_verify_device_u32(const void* dT, uint64_t n, const void* dSA, const void* dLCP,
                                  void* hip_stream, uint64_t* n_errors);
int caps_sa_hip_verify_device_u64(const void* dT, uint64_t n, const void* dSA, const void* dLCP,
                                  void* hip_stream, uint64_t* n_errors);

/* The same checks on a SLICE of the arrays (cnt entries starting anywhere in the suffix array: one rank's share of a
 * sharded build): values in range and none twice within the slice, adjacent order, exact LCP; is_head != 0: entry 0 is
 * the head of the suffix array (its LCP must be 0), else entry 0's LCP is not checked (its predecessor is not in the slice). */
int caps_sa_hip_verify_slice_device_u32(const void* dT, uint64_t n, const void* dSA, const void* dLCP, uint64_t cnt,
                                        int is_head, void* hip_stream, uint64_t* n_errors);
int caps_sa_hip_verify_slice_device_u64(const void* dT, uint64_t n, const void* dSA, const void* dLCP, uint64_t cnt,
                                        int is_head, void* hip_stream, uint64_t* n_errors);

/* ---- Burrows-Wheeler transform, a third result beside SA and LCP ----------------------
 *
 * Let SA be the suffix array the library already builds, in the reference's order. That order includes signed-char bytes and
 * puts a proper prefix before the longer suffix, so it is the order of T·$ with $ below every byte. Then:
 *
 *   BWT[k] = T[(SA[k] + n - 1) mod n] for k in [0, n): n bytes, the text's own bytes as given to the build;
 *   primary = the k with SA[k] == 0.
 *
 * This is the BWT of T·$ with the $ row taken out: L = BWT[primary], BWT[0 .. primary), '$', BWT[primary + 1 .. n) is the last
 * column of the n + 1 sorted rotations of T·$. Nothing else is needed to invert it.
 *
 * For a slice of the SA that does not hold the entry equal to 0, primary comes back as UINT64_MAX (n = 0 included).
 * A bounded-context order (0 < max_context < n) is not a suffix array and has no BWT: CAPS_SA_EUNSUPPORTED.
 */

/* BWT of a slice of a suffix array already in HBM: dBWT[k] = dT[(dSA[k] + n - 1) mod n], k < cnt, where dSA points at rank
 * `first`; *primary = first + k for the k with dSA[k] == 0, else UINT64_MAX.  dT (n bytes), dSA (cnt entries) and dBWT (cnt
 * bytes) are device pointers on the current device; hip_stream as in caps_sa_hip_build_device_*.  first + cnt > n or a null
 * pointer: CAPS_SA_EINVAL.  Returns after the stream work has completed. */
int caps_sa_hip_bwt_device_u32(const void* dT, uint64_t n, const void* dSA, uint64_t first, uint64_t cnt,
                               void* dBWT, void* hip_stream, uint64_t* primary);
int caps_sa_hip_bwt_device_u64(const void* dT, uint64_t n, const void* dSA, uint64_t first, uint64_t cnt,
                               void* dBWT, void* hip_stream, uint64_t* primary);
/* construct() plus the BWT, host buffers: caps_sa_hip_build_* with BWT (n bytes, caller-owned) and *primary.  The BWT leaves the
 * device slice by slice with SA and LCP (stats->result_waves slices; page-locked BWT memory copies at the link rate).  One
 * device only: the sharded builds (caps_sa_hip_build_multi_*) have no BWT output. */
int caps_sa_hip_build_bwt_u32(const char* T, uint64_t n, uint64_t subproblem_count, uint64_t max_context,
                              uint32_t* SA, uint32_t* LCP, uint8_t* BWT, uint64_t* primary, int device, caps_sa_stats* stats);
int caps_sa_hip_build_bwt_u64(const char* T, uint64_t n, uint64_t subproblem_count, uint64_t max_context,
                              uint64_t* SA, uint64_t* LCP, uint8_t* BWT, uint64_t* primary, int device, caps_sa_stats* stats);

/* ---- inverse Burrows-Wheeler transform: the text back from (BWT, primary) --------------
 *
 * The inverse of the block above, over a whole suffix array's (BWT, primary): n bytes and primary < n. Take
 * L = BWT[primary], BWT[0 .. primary), '$', BWT[primary + 1 .. n): rows 0 .. n, bytes in signed-char order, '$' below every
 * byte. F is L sorted, C[c] the symbols of L below c, LF[r] = C[L[r]] + |{r' < r : L[r'] = L[r]}|. Then
 *
 *   T[n - 1 - t] = F[LF^(t+1)(0)] for t in [0, n).
 *
 * LF is a permutation of the n + 1 rows for any input; the input is the BWT of a text exactly when LF is ONE cycle. Any other
 * input is refused with CAPS_SA_EINVAL and a message that says so (T is then unspecified): every input either inverts or gets
 * this error, and every loop of the kernels is bounded by n + 1 steps whatever the input. n = 0: CAPS_SA_OK, nothing read or
 * written (primary not looked at). n >= 1 with primary >= n, a null pointer, n > UINT32_MAX for _u32 (checked before any
 * allocation), a workspace smaller than caps_sa_hip_inverse_bwt_workspace_bytes says: CAPS_SA_EINVAL.
 *
 * The index width sizes the LF table, (n + 1) x 4 bytes for _u32 and x 8 for _u64, plus O(n / 64) for the splitter lists.
 */

/* Workspace of caps_sa_hip_inverse_bwt_device_* for n symbols, idx_bytes = 4 (_u32) or 8 (_u64). */
int caps_sa_hip_inverse_bwt_workspace_bytes(uint64_t n, int idx_bytes, uint64_t* bytes);
/* dBWT (n bytes), dT (n bytes, written) and workspace are device pointers on the current device; the work runs on hip_stream
 * (as in caps_sa_hip_build_device_*). Returns after the stream work has completed: the single-cycle check is read back. */
int caps_sa_hip_inverse_bwt_device_u32(const void* dBWT, uint64_t n, uint64_t primary, void* dT,
                                       void* workspace, uint64_t workspace_bytes, void* hip_stream);
int caps_sa_hip_inverse_bwt_device_u64(const void* dBWT, uint64_t n, uint64_t primary, void* dT,
                                       void* workspace, uint64_t workspace_bytes, void* hip_stream);
/* Host buffers (any host memory; page-locked T copies at the link rate): uploads the BWT, inverts it on `device` and downloads T.
 * Runs on the device block of the host-buffer builds (freed by caps_sa_hip_release_cache(); calls are serialised on it) and
 * restores the caller's current device. */
int caps_sa_hip_inverse_bwt_u32(const uint8_t* BWT, uint64_t n, uint64_t primary, char* T, int device);
int caps_sa_hip_inverse_bwt_u64(const uint8_t* BWT, uint64_t n, uint64_t primary, char* T, int device);

/* ---- FM-index over (BWT, primary): batched count and locate ---------------------------
 *
 * A self-index built from what the build emits, in the row convention of the inverse BWT above (rows 0 .. n of the sorted
 * rotations of T.$, L[0] = BWT[primary], L[primary + 1] = '$', row r >= 1 is SA rank r - 1). It answers "how often does P occur
 * in T" with neither the SA nor the text resident, and "where" from a sparse sample of the SA.
 *
 * Alphabet: at most 4 distinct byte values in the BWT (any bytes, >= 0x80 included), coded 0 .. sigma - 1 in signed-char order --
 * the condition under which the build packs the text to 2 bits. More than 4: CAPS_SA_EALPHABET, decided on the device, nothing
 * written. (A wider alphabet, 1 .. 256 distinct bytes: the wide format below, "FM-index: the wide format", built by
 * caps_sa_hip_fm_build_wide_* and answered by the same count, locate, match and mems calls.)
 *
 * The index is ONE relocatable blob without pointers: copy it device <-> host or write it to a file as it is.
 *   header    256 bytes: magic, format version, n, primary, index width, sigma and the byte values, C[0 .. 4], sa_sample, number of
 *             samples, number of blocks, section offsets, total bytes
 *   Occ       one aligned block per 128 rows (_u32: 64 bytes = 4 x u32 counts | 32 B of 2-bit codes | 16 B of mark bits) or per
 *             256 rows (_u64: 128 bytes = 4 x u64 | 64 B | 32 B): Occ(c, r), the code of a row and its mark touch one block
 *   samples   (only with an SA at build time) per block the number of marked rows before it, then the SA values that are
 *             multiples of sa_sample (a power of two, 1 .. 1024) in row order: sampling by TEXT position bounds every locate
 *             walk by sa_sample LF steps
 * caps_sa_hip_fm_index_bytes(n, 32, 4) = 0.66 n, (n, 32, 8) = 0.78 n, (n, 0, 4) = 0.5 n bytes (+ the header).
 *
 * The blob, byte by byte (format version 1; every number little-endian; version 2 -- "FM-index: extract" below -- appends one
 * section and sets words 1 and 19 .. 22). W = the index width in bytes (4 or 8), ROWS = 128 for
 * W = 4 and 256 for W = 8. The header is 32 64-bit words:
 *   word  0        magic: the 8 bytes "CAPSFMI1" (0x31494D4653504143)
 *   word  1        format version = 1
 *   word  2        n
 *   word  3        primary (0 when n = 0)
 *   word  4        W
 *   word  5        sigma: the number of distinct bytes of the BWT (0 when n = 0)
 *   word  6        the letters, one per byte in code order: bits 8c .. 8c + 7 = the byte of code c, c < sigma; other bytes 0
 *   words 7 .. 11  C[0 .. 4]: C[0] = 1, C[c + 1] = C[c] + the number of bytes of the BWT with code c (codes >= sigma: none),
 *                  so C[4] = n + 1
 *   word  12       sa_sample (0: no samples)
 *   word  13       number of samples = (n - 1) / sa_sample + 1, or 0 when sa_sample = 0 or n = 0
 *   word  14       n_blocks = (n + 1) / ROWS + 1 (integer division): the block of row n + 1 exists
 *   word  15       offset of the Occ section = 256
 *   word  16       offset of the mark ranks = 256 + n_blocks * ROWS / 2
 *   word  17       offset of the samples = word 16 + n_blocks * W rounded up to a multiple of 64 (= word 16 when sa_sample = 0)
 *   word  18       total = word 17 + (number of samples) * W rounded up to a multiple of 64 (= word 17 when sa_sample = 0)
 *   words 19 .. 31 zero
 * Rows: row r of block b = r / ROWS stores a 2-bit code and a mark bit. The STORED code of row 0 is that of BWT[primary], of
 * row r in 1 .. n that of BWT[r - 1], except that the '$' row primary + 1 and the rows behind n (up to n_blocks * ROWS - 1) store
 * code 0. The mark of row r in 1 .. n is 1 iff SA[r - 1] is a multiple of sa_sample; row 0, the rows behind n and every row of
 * an index without samples have mark 0 (the '$' row is SA rank primary, whose SA value 0 is a multiple: its mark is 1).
 * Block b, ROWS / 2 bytes at offset 256 + b * ROWS / 2:
 *   4 counts of W bytes: count[c] = the number of rows before the block (rows 0 .. b * ROWS - 1) whose STORED code is c -- the '$'
 *     row counts as code 0 here; a reader takes it back out of Occ(0, r) for r > primary + 1
 *   ROWS / 16 code words of 32 bits: word i holds rows b * ROWS + 16 i .. + 15, row j of the word at bits 2j, 2j + 1
 *   ROWS / 32 mark words of 32 bits: word i holds rows b * ROWS + 32 i .. + 31, row j of the word at bit j
 * Mark ranks (only with samples): n_blocks numbers of W bytes, mrank[b] = the ABSOLUTE number of marked rows before block b.
 * Samples (only with samples): the SA values that are multiples of sa_sample, W bytes each, in row order (the order in which
 * they stand in the SA). The padding that rounds each of these two sections up to 64 bytes is zero: equal inputs give equal
 * blobs, whatever the memory held before.
 *
 * count: for pattern j = dPatterns[dPatOff[j] .. dPatOff[j + 1]) the occurrences of P in T are exactly SA[first .. first + count)
 * of the library's SA. count == 0 => first == 0 (a byte outside the alphabet included). Empty pattern: first = 0, count = n. A
 * pattern longer than n: 0.
 * locate: for query j and t < min(dCount[j], dOutOff[j + 1] - dOutOff[j]): dPos[dOutOff[j] + t] = SA[dFirst[j] + t] -- SA order,
 * comparable with the SA entry by entry; a caller that wants at most k hits per query sizes the offsets so. Other slots of dPos
 * are not written by the device form and come back as UINT64_MAX from the host form. An index built without an SA counts, and
 * answers locate with CAPS_SA_EUNSUPPORTED.
 *
 * Errors: the header is read back and checked on the HOST (magic, version, width, primary < n for n >= 1, C[], section offsets
 * and total against index_bytes) before any kernel reads the body: anything wrong is CAPS_SA_EINVAL with a message in
 * caps_sa_hip_last_error(). Non-monotone dPatOff / dOutOff, first + count > n, a null pointer with q > 0: CAPS_SA_EINVAL. n = 0:
 * the build succeeds and every count is 0. n > UINT32_MAX with _u32: CAPS_SA_EINVAL before any allocation. The kernels compare
 * every row, block and sample index with its section's size before it is used: for any body they read inside the blob and
 * terminate (count: at most one step per pattern byte; locate: at most sa_sample steps). A locate walk that does not end within
 * sa_sample steps means the blob is not an index this library built: CAPS_SA_EINVAL, the message says so, dPos unspecified.
 */

/* Size of the index of n symbols: sa_sample = 0 for an index without samples, idx_bytes = 4 (_u32) or 8 (_u64). */
int caps_sa_hip_fm_index_bytes(uint64_t n, uint32_t sa_sample, int idx_bytes, uint64_t* bytes);
/* dBWT (n bytes), dSA (NULL: no samples, sa_sample ignored; else the WHOLE suffix array, n entries of the index width) and dIndex
 * (index_bytes >= caps_sa_hip_fm_index_bytes, written; 64-byte aligned) are device pointers on the current device; the work runs
 * on hip_stream and has completed on return. An SA whose multiples of sa_sample are not (n - 1) / sa_sample + 1: CAPS_SA_EINVAL. */
int caps_sa_hip_fm_build_device_u32(const void* dBWT, uint64_t n, uint64_t primary, const void* dSA, uint32_t sa_sample,
                                    void* dIndex, uint64_t index_bytes, void* hip_stream);
int caps_sa_hip_fm_build_device_u64(const void* dBWT, uint64_t n, uint64_t primary, const void* dSA, uint32_t sa_sample,
                                    void* dIndex, uint64_t index_bytes, void* hip_stream);
/* Host buffers: BWT and SA (or NULL) up, the index built on `device` and downloaded into `index`. Runs on the device block of the
 * host-buffer builds (calls serialised on it, the caller's current device restored); the index stays there for the host queries. */
int caps_sa_hip_fm_build_u32(const uint8_t* BWT, uint64_t n, uint64_t primary, const uint32_t* SA, uint32_t sa_sample,
                             void* index, uint64_t index_bytes, int device);
int caps_sa_hip_fm_build_u64(const uint8_t* BWT, uint64_t n, uint64_t primary, const uint64_t* SA, uint32_t sa_sample,
                             void* index, uint64_t index_bytes, int device);
/* dPatOff: u64[q + 1], dFirst / dCount: u64[q] (written), all on the current device; the index width comes from the header. */
int caps_sa_hip_fm_count_device(const void* dIndex, uint64_t index_bytes, const void* dPatterns, const void* dPatOff, uint64_t q,
                                void* dFirst, void* dCount, void* hip_stream);
/* dFirst / dCount: u64[q] (e.g. what count wrote), dOutOff: u64[q + 1], dPos: u64[dOutOff[q]] (written). */
int caps_sa_hip_fm_locate_device(const void* dIndex, uint64_t index_bytes, const void* dFirst, const void* dCount,
                                 const void* dOutOff, uint64_t q, void* dPos, void* hip_stream);
/* The same on host buffers, the index in host memory: it is uploaded to the device block of the host-buffer builds (calls
 * serialised on it, the caller's current device restored), and an index already uploaded is not uploaded again. "Already
 * uploaded" = same address, size, header and the same sum over a stride of the body: a caller that rewrites a blob in place
 * calls caps_sa_hip_release_cache() before it queries again. */
int caps_sa_hip_fm_count(const void* index, uint64_t index_bytes, const uint8_t* patterns, const uint64_t* pat_off, uint64_t q,
                         uint64_t* first, uint64_t* count, int device);
int caps_sa_hip_fm_locate(const void* index, uint64_t index_bytes, const uint64_t* first, const uint64_t* count,
                          const uint64_t* out_off, uint64_t q, uint64_t* pos, int device);

/* ---- FM-index from the BWT alone: the SA samples by LF walk -----------------------------
 *
 * The same blob as caps_sa_hip_fm_build_* with an SA, for a caller who holds (BWT, primary) and nothing else: dIndex receives
 * exactly the bytes that caps_sa_hip_fm_build_device_* writes for (BWT, primary, SA, sa_sample), where SA is the suffix array of
 * the text that this BWT inverts to. With the rows of the inverse BWT above, LF^k(0) for k = 1 .. n is the row of the suffix at
 * text position n - k (k = n: the '$' row, position 0), so a row's offset on the LF cycle of row 0 is its SA value. The Occ section
 * is built first and gives LF in one block per step; the rows 0 mod 64 cut the cycle into segments, the list of segments is ranked
 * by the inverse BWT's list levels, and a second walk marks the rows whose position is a multiple of sa_sample. Neither the text nor
 * the SA exists at any time.
 *
 * sa_sample: a power of two in 1 .. 1024. 0 is CAPS_SA_EINVAL (an index without samples: caps_sa_hip_fm_build_* with a null SA).
 * Workspace: caps_sa_hip_fm_from_bwt_workspace_bytes(n, sa_sample, W) <= (number of samples) * W + 32 * (n / 64 + 1) + 2^20 bytes, W
 * the index width -- no array of n entries. A NULL workspace is allocated and freed by the call; one that is too small is
 * CAPS_SA_EINVAL. Errors, all CAPS_SA_EINVAL and checked before any allocation: a null pointer (dBWT may be null for n = 0),
 * primary >= n for n >= 1, n > UINT32_MAX with _u32, index_bytes below caps_sa_hip_fm_index_bytes(n, sa_sample, W). More than 4
 * distinct bytes: CAPS_SA_EALPHABET, decided before anything is written to the index. n = 0 succeeds: the blob of the format table,
 * no samples and sa_sample in word 12. A (BWT, primary) that is not the BWT of any text (its LF mapping is not one cycle) is
 * CAPS_SA_EINVAL with the message of the inverse BWT; the contents of the index are then unspecified. Every loop of the kernels is
 * bounded by n + 1 steps whatever the input.
 */

/* Workspace of caps_sa_hip_fm_build_from_bwt_device_*, idx_bytes = 4 (_u32) or 8 (_u64). */
int caps_sa_hip_fm_from_bwt_workspace_bytes(uint64_t n, uint32_t sa_sample, int idx_bytes, uint64_t* bytes);
/* dBWT (n bytes), dIndex (index_bytes >= caps_sa_hip_fm_index_bytes(n, sa_sample, W), written; 64-byte aligned) and workspace (or
 * NULL) are device pointers on the current device; the work runs on hip_stream and has completed on return (the alphabet, the
 * symbol totals and the single-cycle check are read back). */
int caps_sa_hip_fm_build_from_bwt_device_u32(const void* dBWT, uint64_t n, uint64_t primary, uint32_t sa_sample,
                                             void* dIndex, uint64_t index_bytes, void* workspace, uint64_t workspace_bytes, void* hip_stream);
int caps_sa_hip_fm_build_from_bwt_device_u64(const void* dBWT, uint64_t n, uint64_t primary, uint32_t sa_sample,
                                             void* dIndex, uint64_t index_bytes, void* workspace, uint64_t workspace_bytes, void* hip_stream);
/* Host buffers: the BWT up, the index built on `device` and downloaded into `index`. Runs on the device block of the host-buffer
 * builds (calls serialised on it, the caller's current device restored); the index stays there for the host queries. */
int caps_sa_hip_fm_build_from_bwt_u32(const uint8_t* BWT, uint64_t n, uint64_t primary, uint32_t sa_sample,
                                      void* index, uint64_t index_bytes, int device);
int caps_sa_hip_fm_build_from_bwt_u64(const uint8_t* BWT, uint64_t n, uint64_t primary, uint32_t sa_sample,
                                      void* index, uint64_t index_bytes, int device);

/* ---- FM-index: extract -- text substrings from the index alone ---------------------------
 *
 * extract(i, l) = T[i .. i + l), the third operation of a self-index: a caller who keeps only the blob can show the flanks of a hit,
 * verify a match or cut a window of the text, without the text and without inverting the whole BWT. The stored code of the row of
 * the suffix at text position e is T[e - 1] and LF leads from that row to the row of the suffix at e - 1, so the text is read
 * DOWNWARDS from any position whose row is known. Format version 2 adds those rows for every text_sample-th position.
 *
 * The blob, format version 2: a version-1 blob WITH samples plus one section behind it. Words 0 and 2 .. 18 and every byte of the
 * Occ, mark-rank and sample sections are those of version 1 (word 18 keeps its meaning: the end of the version-1 sections).
 *   word  1        format version = 2
 *   word  19       text_sample t: a power of two with sa_sample <= t <= 1024
 *   word  20       m = number of text samples = (n - 1) / t + 1 (0 when n = 0)
 *   word  21       offset of the section = word 18
 *   word  22       total = word 21 + m * W rounded up to a multiple of 64
 *   words 23 .. 31 zero
 * Section: rowof[k], W bytes each, k = 0 .. m - 1: the row, in 1 .. n, of the suffix that starts at text position k * t (1 + its
 * SA rank), so rowof[0] = primary + 1. The padding is zero. count and locate give on a version-2 blob what they give on its
 * version-1 part; a reader of version 1 refuses version 2 by its version word.
 *
 * caps_sa_hip_fm_add_text_samples_*: in place, a version-1 blob WITH samples becomes version 2 (a version-2 blob: its section is
 * rebuilt at the new distance). The section comes from the blob itself -- a marked row r carries the sample v = samples[mrank[block]
 * + marks below r in its block]; v a multiple of t gives rowof[v / t] = r; sa_sample divides t, so every multiple of t is a sample
 * -- in one pass over the mark words and the samples: the same call serves blobs built with the SA, from the BWT alone, or read
 * from a file. index_bytes is the CAPACITY of the buffer: below caps_sa_hip_fm_index_bytes_ex(n, sa_sample, t, W) is
 * CAPS_SA_EINVAL with nothing written. An index without samples: CAPS_SA_EUNSUPPORTED. t not a power of two in sa_sample .. 1024:
 * CAPS_SA_EINVAL. n = 0 succeeds with m = 0. A blob whose samples leave a rowof slot empty or outside 1 .. n (a sample missing or
 * twice: not an index this library built) is CAPS_SA_EINVAL and its header says version 1. The host form rewrites the caller's blob
 * (header and section) and leaves the device copy of the host queries equal to it.
 *
 * caps_sa_hip_fm_extract_*: query j asks for len_j = dOutOff[j + 1] - dOutOff[j] bytes from text position dStart[j]:
 *   dText[dOutOff[j] .. dOutOff[j + 1]) = T[dStart[j] .. dStart[j] + len_j)
 * as the original letters (header word 6). The positions are cut into chunks [k t, (k + 1) t); one GPU lane serves one (query,
 * chunk) pair, starts at the chunk's upper end E = min((k + 1) t, n) in row rowof[k + 1] (row 0 for E = n: no sample is needed at
 * the text's end) and takes at most t LF steps, one Occ block each, down to max(k t, start): a query of length l costs about
 * l + t steps on l / t + 1 lanes, and extract(0, n) runs over the whole GPU. Bytes of dText outside every range are not written.
 * Workspace: caps_sa_hip_fm_extract_workspace_bytes(q) = 8 (q + 1) bytes and alignment slack, the scanned chunk counts; NULL is
 * allocated and freed by the call. Errors: the header is checked on the host as for count; a version-1 blob is
 * CAPS_SA_EUNSUPPORTED; non-monotone dOutOff, start + len > n (computed without overflow), a null pointer with q > 0, a workspace
 * that is too small: CAPS_SA_EINVAL with nothing written. q = 0 and a batch of empty ranges succeed. The kernel compares every row,
 * block and rowof index with its section's size before it is used; a walk that meets the '$' row or row 0 below its sample means
 * the blob is not an index this library built: CAPS_SA_EINVAL, dText unspecified.
 */

/* Size of a version-2 index: sa_sample a power of two in 1 .. 1024, text_sample a power of two in sa_sample .. 1024. */
int caps_sa_hip_fm_index_bytes_ex(uint64_t n, uint32_t sa_sample, uint32_t text_sample, int idx_bytes, uint64_t* bytes);
/* dIndex: a device pointer on the current device, index_bytes its capacity; runs on hip_stream and has completed on return. */
int caps_sa_hip_fm_add_text_samples_device(void* dIndex, uint64_t index_bytes, uint32_t text_sample, void* hip_stream);
/* The same on a blob in host memory (index_bytes: the capacity of the buffer), on the device block of the host-buffer builds. */
int caps_sa_hip_fm_add_text_samples(void* index, uint64_t index_bytes, uint32_t text_sample, int device);
int caps_sa_hip_fm_extract_workspace_bytes(uint64_t q, uint64_t* bytes);
/* dStart: u64[q], dOutOff: u64[q + 1], dText: u8[dOutOff[q]] (written), workspace (or NULL): device pointers on the current device. */
int caps_sa_hip_fm_extract_device(const void* dIndex, uint64_t index_bytes, const void* dStart, const void* dOutOff, uint64_t q,
                                  void* dText, void* workspace, uint64_t workspace_bytes, void* hip_stream);
/* The same on host buffers; the index is uploaded as for caps_sa_hip_fm_count. text[out_off[0] .. out_off[q]) is written. */
int caps_sa_hip_fm_extract(const void* index, uint64_t index_bytes, const uint64_t* start, const uint64_t* out_off, uint64_t q,
                           uint8_t* text, int device);

/* ---- FM-index: matching statistics and maximal exact matches ------------------------------
 *
 * count answers for a whole pattern; a read with one wrong base counts 0. The seeding question of a read mapper is asked for every
 * position instead. Let P be a pattern of m bytes and T the indexed text. For an END e in 1 .. m:
 *   L[e]                 the largest l <= e such that P[e - l .. e) occurs in T (0 when P[e - 1] is no letter of the index); with a
 *                        cap max_len > 0 additionally l <= max_len
 *   (first[e], count[e]) the SA interval of P[e - L[e] .. e) in count's convention: the occurrences are SA[first .. first + count).
 *                        L[e] = 0 gives first = count = 0 (not the empty pattern's (0, n)).
 * Without a cap L[e + 1] <= L[e] + 1, and the match ending at e is left-maximal by construction. It is a maximal exact match (MEM)
 * iff L[e] >= 1 and e = m, or P[e] is no letter, or L[e + 1] <= L[e]; every MEM of P against T arises so, exactly once. (P[e] no
 * letter gives L[e + 1] = 0: the third condition covers the second.)
 *
 * Nothing is read but the Occ blocks, C[] and the '$' row: both calls work on version-1 and version-2 blobs, with or without SA
 * samples. One GPU lane serves one (pattern, end) pair and runs count's backward search from byte e - 1 leftwards, both LF
 * lookups of a step issued together, until the interval is empty, a byte is no letter, the pattern's first byte is passed or
 * max_len steps are done: at most min(e, max_len) steps for any blob body, every row and block clamped as in count.
 *
 * total = dPatOff[q] - dPatOff[0]; output slot dPatOff[j] - dPatOff[0] + e - 1 belongs to end e of pattern j. dLen is u32[total];
 * dFirst / dCount are u64[total] each, or NULL (each on its own): not written.
 *
 * caps_sa_hip_fm_mems_*: the MEMs of at least min_len bytes (0 is treated as 1), without a cap, as records of 32 bytes
 *   u64 pattern index | u32 start within the pattern | u32 length | u64 first | u64 count          (little-endian)
 * in (pattern, increasing end) order; dMemOff[j] .. dMemOff[j + 1] are the records of pattern j (u64[q + 1], always written).
 * dMems = NULL is the counting call: only dMemOff is written. dMems non-null (8-byte aligned) with dMemOff[q] > mem_capacity
 * (in records) is CAPS_SA_EINVAL: dMemOff is still valid and no record is written. Workspace:
 * caps_sa_hip_fm_mems_workspace_bytes(total, q) -- 28 bytes per pattern byte (lengths, intervals, record slots) and at most
 * 24 KiB; NULL is allocated and freed by the call.
 *
 * Errors follow count's: the header is checked on the host first; a null pointer with q > 0 and non-monotone offsets are
 * CAPS_SA_EINVAL, and so is a pattern longer than 2^32 - 1 bytes. q = 0 succeeds (dMemOff[0] = 0). n = 0: every length is 0 and
 * there are no MEMs.
 */
int caps_sa_hip_fm_match_device(const void* dIndex, uint64_t index_bytes, const void* dPatterns, const void* dPatOff, uint64_t q,
                                uint32_t max_len, void* dLen, void* dFirst, void* dCount, void* hip_stream);
/* The same on host buffers; the index is uploaded as for caps_sa_hip_fm_count. */
int caps_sa_hip_fm_match(const void* index, uint64_t index_bytes, const uint8_t* patterns, const uint64_t* pat_off, uint64_t q,
                         uint32_t max_len, uint32_t* len, uint64_t* first, uint64_t* count, int device);
int caps_sa_hip_fm_mems_workspace_bytes(uint64_t total_pattern_bytes, uint64_t q, uint64_t* bytes);
int caps_sa_hip_fm_mems_device(const void* dIndex, uint64_t index_bytes, const void* dPatterns, const void* dPatOff, uint64_t q,
                               uint32_t min_len, void* dMemOff, void* dMems, uint64_t mem_capacity, void* workspace,
                               uint64_t workspace_bytes, void* hip_stream);
int caps_sa_hip_fm_mems(const void* index, uint64_t index_bytes, const uint8_t* patterns, const uint64_t* pat_off, uint64_t q,
                        uint32_t min_len, uint64_t* mem_off, void* mems, uint64_t mem_capacity, int device);

/* ---- FM-index: the wide format -- count, locate and MEMs over any bytes -----------------
 *
 * A second blob format for a BWT of 1 .. 256 distinct bytes (a genome with N, IUPAC DNA, protein, any text), built from
 * (BWT, primary[, SA]) by caps_sa_hip_fm_build_wide_* and answered by caps_sa_hip_fm_count*, _locate*, _match* and _mems* above, which
 * tell the two formats apart by the magic; their contracts are unchanged. caps_sa_hip_fm_add_text_samples*, _extract* and
 * caps_sa_hip_fm_build_from_bwt* are not built for it: the first two answer a wide blob with CAPS_SA_EUNSUPPORTED and write nothing.
 *
 * The rank structure is a 4-ary wavelet matrix made of version 1's Occ blocks. Letters are coded 0 .. sigma - 1 in signed-char
 * order; a code is written with Lv = max(1, ceil(log4 sigma)) base-4 digits, digit 0 the most significant (Lv = 2 for ACGTN and
 * IUPAC, 3 for protein, 4 for all bytes). Rows are version 1's: rows 0 .. n, row 0 carries BWT[primary], row r in 1 .. n BWT[r - 1],
 * the '$' row primary + 1 is STORED AS CODE 0. Level 0 is the code sequence in row order; level l + 1 is level l stably partitioned
 * by its level-l digit (all rows with digit 0 first, then 1, 2, 3). With
 *   Occ_l(d, p)  the rows below position p of level l whose digit is d
 *   Z[l][d]      the rows 0 .. n of level l with a digit below d
 *   zone[c]      the position that code c reaches from p = 0
 * the LF step is
 *   p = r;  for l in 0 .. Lv - 1:  d = digit_l(c);  p = Z[l][d] + Occ_l(d, p)
 *   LF(c, r) = C[c] + p - zone[c] - [c == 0 and r > primary + 1]
 * and the code of a row (locate) comes from the same descent with the digit AT p in the place of digit_l(c): one aligned block
 * per level and step. sigma <= 4 gives Lv = 1, and the level-0 section is then byte for byte the Occ section of version 1.
 *
 * The blob, byte by byte (wide format version 1; little-endian; W, ROWS as in version 1). The header is 32 64-bit words:
 *   word  0        magic: the 8 bytes "CAPSFMW1" (0x31574D4653504143)
 *   word  1        format version = 1
 *   words 2 .. 4   n, primary (0 when n = 0), W                                          -- version 1's words
 *   word  5        sigma: the number of distinct bytes of the BWT, 0 .. 256 (0 when n = 0)
 *   word  6        Lv
 *   word  7        offset of the table section = 256
 *   word  8        bytes of one level section = n_blocks * ROWS / 2
 *   words 9 .. 11  zero
 *   words 12 .. 14 sa_sample (0: no samples), number of samples, n_blocks              -- version 1's words and rules
 *   word  15       offset of level 0 = 256 + 4800; level l stands at word 15 + l * word 8
 *   word  16       offset of the mark ranks = word 15 + Lv * word 8
 *   word  17       offset of the samples = word 16 + n_blocks * W rounded up to a multiple of 64 (= word 16 when sa_sample = 0)
 *   word  18       total = word 17 + (number of samples) * W rounded up to a multiple of 64 (= word 17 when sa_sample = 0)
 *   words 19 .. 31 zero
 * Table section, 4800 bytes at offset 256 (offsets within the section):
 *   0     letters u8[256]: letters[c] = the byte of code c for c < sigma, else 0
 *   256   code_of u8[256]: code_of[b] = the number of letters below byte b in signed-char order. b is a letter iff
 *         code_of[b] < sigma and letters[code_of[b]] == b: there is no sentinel value
 *   512   C u64[257]: C[0] = 1, C[c + 1] = C[c] + the number of bytes of the BWT with code c, so C[c] = n + 1 for c >= sigma
 *   2568  zone u64[256] (0 for c >= sigma)
 *   4616  Z u64[4][4]: Z[l][d] at 4616 + 8 (4 l + d); rows l >= Lv are 0
 *   4744  56 zero bytes
 *   (n = 0: every C[c] = 1, everything else in the section 0.)
 * Level sections: each is an Occ section in version 1's block layout -- per block 4 counts of W bytes (the rows of the level
 * before the block whose digit is 0, 1, 2, 3), ROWS / 16 words of 2-bit digits, ROWS / 32 mark words. Only level 0 carries marks
 * (version 1's: row r is marked iff SA[r - 1] is a multiple of sa_sample); the mark words of the other levels are 0. Positions
 * behind n store digit 0 and are in no count. Mark ranks and samples: as in version 1, present only with an SA. All padding is 0:
 * equal inputs give equal blobs. Size: Lv * 0.5 n + 0.16 n bytes at sa_sample = 32, W = 4.
 *
 * Build: dSA NULL builds an index that counts (sa_sample ignored). The alphabet is found on the device, so the blob's size is known
 * only afterwards: it is header word 18. index_capacity must hold it -- caps_sa_hip_fm_wide_index_bytes(n, sigma, ..), sigma = 0
 * for "unknown" (sized for 256 letters). Workspace: caps_sa_hip_fm_wide_workspace_bytes(n, W) = two code buffers of n + 1 bytes and
 * 40 bytes per 16,384 rows (+ 2.1 MB): no array of n index entries; NULL is allocated and freed by the call.
 * Errors, CAPS_SA_EINVAL and checked before any allocation: a null pointer (dBWT may be null for n = 0), primary >= n for n >= 1,
 * n > UINT32_MAX with _u32, sa_sample no power of two in 1 .. 1024 with an SA, a workspace that is too small, an index_capacity
 * below the smallest index of n symbols; a capacity below the blob of the alphabet found is CAPS_SA_EINVAL too, with nothing
 * written. An SA whose multiples of sa_sample are not (n - 1) / sa_sample + 1: CAPS_SA_EINVAL. n = 0
 * builds, and counts 0.
 *
 * Queries: header AND table section are read back and checked on the host before a kernel reads the body -- the letters ascending,
 * code_of, C monotone from 1 to n + 1, zone and Z recomputed from C, every offset recomputed, total <= index_bytes: anything wrong
 * is CAPS_SA_EINVAL. The kernels keep every position inside 0 .. n + 1 and every block inside its level at every level, and every
 * loop is bounded as in version 1: for any body they read inside the blob and terminate.
 */
int caps_sa_hip_fm_wide_index_bytes(uint64_t n, uint32_t sigma, uint32_t sa_sample, int idx_bytes, uint64_t* bytes);
int caps_sa_hip_fm_wide_workspace_bytes(uint64_t n, int idx_bytes, uint64_t* bytes);
/* dBWT (n bytes), dSA (NULL or the whole suffix array), dIndex (index_capacity bytes, 64-byte aligned, written) and workspace (or
 * NULL) are device pointers on the current device; the work runs on hip_stream and has completed on return. */
int caps_sa_hip_fm_build_wide_device_u32(const void* dBWT, uint64_t n, uint64_t primary, const void* dSA, uint32_t sa_sample,
                                         void* dIndex, uint64_t index_capacity, void* workspace, uint64_t workspace_bytes, void* hip_stream);
int caps_sa_hip_fm_build_wide_device_u64(const void* dBWT, uint64_t n, uint64_t primary, const void* dSA, uint32_t sa_sample,
                                         void* dIndex, uint64_t index_capacity, void* workspace, uint64_t workspace_bytes, void* hip_stream);
/* Host buffers, on the device block of the host-buffer builds as caps_sa_hip_fm_build_*: header word 18 bytes of `index` are written. */
int caps_sa_hip_fm_build_wide_u32(const uint8_t* BWT, uint64_t n, uint64_t primary, const uint32_t* SA, uint32_t sa_sample,
                                  void* index, uint64_t index_capacity, int device);
int caps_sa_hip_fm_build_wide_u64(const uint8_t* BWT, uint64_t n, uint64_t primary, const uint64_t* SA, uint32_t sa_sample,
                                  void* index, uint64_t index_capacity, int device);

/* ---- k-mers from SA and LCP ---------------------------------------------------------
 * The k-mer table, the multiplicity spectrum and a census over every k of a text, from the two arrays a full-context construct()
 * gives and nothing else: the text is not read. T is a text of n bytes, SA its suffix array, LCP[i] the exact common prefix of the
 * suffixes SA[i - 1] and SA[i]; LCP[0] counts as 0 whatever it holds. k >= 1.
 *   - Rank i is a HEAD iff i == 0 or LCP[i] < k.
 *   - The RUN of a head h is the ranks h .. h' - 1, h' the next head, or n if there is none.
 *   - A run IS A K-MER iff SA[h] <= n - k (computed without overflow; for k > n no run is a k-mer). Its bytes are
 *     T[SA[h] .. SA[h] + k), its count is h' - h, its occurrences are SA[h .. h').
 *   - A suffix shorter than k is always a run of its own and is no k-mer.
 *   - The runs in rank order are the distinct k-mers in the library's byte order (the reference's signed-char order).
 * The cost does not depend on k, and the table comes out sorted.
 *
 * Arrays of a bounded-context build (max_context > 0) are not a suffix array: the result is then unspecified. For arrays that are
 * not the SA / LCP of any text the calls still terminate, read only SA[0 .. n) and LCP[0 .. n) and write only inside the output
 * buffers: nothing is indexed by a value read from the arrays except histogram bins, and those are clamped. There is no validation
 * pass and no error for such inputs.
 *
 * kmers: the k-mers with min_count <= count <= max_count (min_count = 0 is treated as 1, max_count = 0 means no upper bound,
 * min_count > max_count > 0 is CAPS_SA_EINVAL) as records of 24 bytes, little-endian, in rank order:
 *     u64 first (the head's rank) | u64 count | u64 pos (SA[first])
 * *n_records (host) is always written. dRecords = NULL is the counting call. A non-null dRecords (8-byte aligned) with
 * *n_records > capacity is CAPS_SA_EINVAL: *n_records is still valid and no record is written.
 *
 * kmer_spectrum: hist (host, u64[bins + 1]): hist[c], 1 <= c < bins, = the distinct k-mers that occur exactly c times,
 * hist[bins] = those that occur bins times or more, hist[0] = 0. bins in 1 .. 1024.
 *
 * kmer_census: every k in 1 .. max_k (max_k in 1 .. 1024) from one pass: distinct[k] = the number of distinct k-mers, unique[k] =
 * the number that occur once (host, u64[max_k + 1] each; index 0 is 0). Per rank i, with a = (i == 0 ? 0 : LCP[i]),
 * a' = max(a, i + 1 < n ? LCP[i + 1] : 0) and b = (SA[i] < n ? n - SA[i] : 0): rank i adds 1 to distinct[k] for a < k <= b and to
 * unique[k] for a' < k <= b.
 *
 * Common: k = 0, max_k = 0, a null pointer with n > 0, n > UINT32_MAX with _u32 or a workspace that is too small are
 * CAPS_SA_EINVAL, checked before any allocation, nothing written. n = 0 succeeds with zeros. The workspace
 * (caps_sa_hip_kmer_workspace_bytes) is O(n / 16,384) words and a fixed 16.8 MB of histogram columns, no array of n entries; NULL
 * is allocated and freed by the call. dSA, dLCP, dRecords and workspace are device pointers on the current device; the work runs on
 * hip_stream and has completed on return. Ranks beyond 2^32 (_u64 with n > UINT32_MAX) are untested.
 */
int caps_sa_hip_kmer_workspace_bytes(uint64_t n, int idx_bytes, uint64_t* bytes);
int caps_sa_hip_kmers_device_u32(const void* dSA, const void* dLCP, uint64_t n, uint64_t k, uint64_t min_count, uint64_t max_count,
                                 void* dRecords, uint64_t capacity, uint64_t* n_records, void* workspace, uint64_t workspace_bytes,
                                 void* hip_stream);
int caps_sa_hip_kmers_device_u64(const void* dSA, const void* dLCP, uint64_t n, uint64_t k, uint64_t min_count, uint64_t max_count,
                                 void* dRecords, uint64_t capacity, uint64_t* n_records, void* workspace, uint64_t workspace_bytes,
                                 void* hip_stream);
int caps_sa_hip_kmer_spectrum_device_u32(const void* dSA, const void* dLCP, uint64_t n, uint64_t k, uint32_t bins, uint64_t* hist,
                                         void* workspace, uint64_t workspace_bytes, void* hip_stream);
int caps_sa_hip_kmer_spectrum_device_u64(const void* dSA, const void* dLCP, uint64_t n, uint64_t k, uint32_t bins, uint64_t* hist,
                                         void* workspace, uint64_t workspace_bytes, void* hip_stream);
int caps_sa_hip_kmer_census_device_u32(const void* dSA, const void* dLCP, uint64_t n, uint32_t max_k, uint64_t* distinct,
                                       uint64_t* unique, void* workspace, uint64_t workspace_bytes, void* hip_stream);
int caps_sa_hip_kmer_census_device_u64(const void* dSA, const void* dLCP, uint64_t n, uint32_t max_k, uint64_t* distinct,
                                       uint64_t* unique, void* workspace, uint64_t workspace_bytes, void* hip_stream);
/* Host SA and LCP (and host records): the arrays go up into device buffers of the call's own on `device`, the records come down. */
int caps_sa_hip_kmers_u32(const uint32_t* SA, const uint32_t* LCP, uint64_t n, uint64_t k, uint64_t min_count, uint64_t max_count,
                          void* records, uint64_t capacity, uint64_t* n_records, int device);
int caps_sa_hip_kmers_u64(const uint64_t* SA, const uint64_t* LCP, uint64_t n, uint64_t k, uint64_t min_count, uint64_t max_count,
                          void* records, uint64_t capacity, uint64_t* n_records, int device);
int caps_sa_hip_kmer_spectrum_u32(const uint32_t* SA, const uint32_t* LCP, uint64_t n, uint64_t k, uint32_t bins, uint64_t* hist,
                                  int device);
int caps_sa_hip_kmer_spectrum_u64(const uint64_t* SA, const uint64_t* LCP, uint64_t n, uint64_t k, uint32_t bins, uint64_t* hist,
                                  int device);
int caps_sa_hip_kmer_census_u32(const uint32_t* SA, const uint32_t* LCP, uint64_t n, uint32_t max_k, uint64_t* distinct,
                                uint64_t* unique, int device);
int caps_sa_hip_kmer_census_u64(const uint64_t* SA, const uint64_t* LCP, uint64_t n, uint32_t max_k, uint64_t* distinct,
                                uint64_t* unique, int device);

/* ---- LPF and LZ77 from SA and LCP ---------------------------------------------------
 * The longest-previous-factor array with a previous occurrence for every position, and the LZ77 factorization that follows from
 * it, from the two arrays a full-context construct() gives: the text is not read. n entries; SA is a permutation of 0 .. n - 1; LCP
 * is any array, and LCP[0] counts as 0 whatever it holds. For rank r with i = SA[r]:
 *   - p = the largest rank < r with SA[p] < i. If there is one, left = min(LCP[p + 1 .. r]); if there is none, left = 0.
 *   - q = the smallest rank > r with SA[q] < i. If there is one, right = min(LCP[r + 1 .. q]); if there is none, right = 0.
 *   - LPF[i] = max(left, right).
 *   - Prev[i] = SA[p] if left >= right and left > 0; Prev[i] = SA[q] if right > left; Prev[i] = the all-ones value of the index
 *     width if LPF[i] = 0. On equal lengths the lower-rank side wins.
 * When (SA, LCP) are the arrays of a full-context build of T, LPF[i] is the longest prefix of T[i ..) that also starts at some j < i
 * (the two may overlap), Prev[i] is such a j, and LPF[i] <= n - i. Arrays of a bounded-context build are no suffix array: the
 * result is then unspecified.
 *
 * lpf: dLPF and dPrev are n entries of the index width in TEXT order; either may be NULL and is then not written (both NULL with
 * n > 0 is CAPS_SA_EINVAL). A value SA[r] >= n is never used as an index: that rank is skipped, the call returns CAPS_SA_EINVAL
 * ("not a suffix array") and its outputs are unspecified. Duplicate SA values are not detected; a slot whose position never occurs
 * in SA keeps what it held. The work per rank is bounded for ANY permutation: at most 2 * 64 steps per level of a 64-ary tree of
 * (min SA, min LCP) summaries over the ranks and per direction, 2 + ceil(log64(n / 4096)) levels.
 *
 * LZ77 from (LPF, Prev), both in text order: s_0 = 0; the phrase at s has len = min(max(1, LPF[s]), n - s) and src = Prev[s] if
 * LPF[s] > 0, else UINT64_MAX (a literal of one byte); s_{j+1} = s_j + len_j until s = n. Records of 24 bytes, little-endian, in
 * text order:
 *     u64 pos | u64 len | u64 src
 * z = the number of records. The clamp makes the chain defined for any arrays, and it moves strictly forward.
 * *n_phrases (host) is always written. dRecords = NULL is the counting call. A non-null dRecords (8-byte aligned) with
 * *n_phrases > capacity is CAPS_SA_EINVAL: *n_phrases is still valid and no record is written.
 *
 * Common: a null array with n > 0, a null n_phrases, n > UINT32_MAX with _u32 or a workspace that is too small are CAPS_SA_EINVAL,
 * checked before any allocation, nothing written. n = 0 succeeds with z = 0. For any input every call terminates and reads and
 * writes only inside its arrays. Workspaces (W = the index width in bytes; NULL is allocated and freed by the call):
 *   lpf   no array of n entries: 2 W (ceil(n / 64) + ceil(n / 64^2) + ... + 1) bytes of summaries, each array rounded up to 256
 *         bytes, plus 1,024 bytes (the level table, the flag, alignment) -- less than n W / 31 + 2 KiB;
 *   lz77  one array of n entries of the index width (where the chain from every position leaves its tile of 16,384). Exactly, with
 *         t = ceil(n / 16,384) tiles, g = ceil(n / 1,048,576) groups of 64 tiles and up(b) = b rounded up to 256:
 *         up(n W) + up(64 g W) + up(8 g) + up(8 t) + up(8 (t + 1)) + 512 bytes.
 * (lpf exactly: 2 up(W nodes) + 1,024 with nodes = ceil(n / 64) + ceil(n / 64^2) + ... + 1.)
 * dSA, dLCP, dLPF, dPrev, dRecords and workspace are device pointers on the current device; the work runs on hip_stream and has
 * completed on return. Ranks beyond 2^32 (_u64 with n > UINT32_MAX) are untested.
 */
int caps_sa_hip_lpf_workspace_bytes(uint64_t n, int idx_bytes, uint64_t* bytes);
int caps_sa_hip_lpf_device_u32(const void* dSA, const void* dLCP, uint64_t n, void* dLPF, void* dPrev, void* workspace,
                               uint64_t workspace_bytes, void* hip_stream);
int caps_sa_hip_lpf_device_u64(const void* dSA, const void* dLCP, uint64_t n, void* dLPF, void* dPrev, void* workspace,
                               uint64_t workspace_bytes, void* hip_stream);
int caps_sa_hip_lz77_workspace_bytes(uint64_t n, int idx_bytes, uint64_t* bytes);
int caps_sa_hip_lz77_device_u32(const void* dLPF, const void* dPrev, uint64_t n, void* dRecords, uint64_t capacity, uint64_t* n_phrases,
                                void* workspace, uint64_t workspace_bytes, void* hip_stream);
int caps_sa_hip_lz77_device_u64(const void* dLPF, const void* dPrev, uint64_t n, void* dRecords, uint64_t capacity, uint64_t* n_phrases,
                                void* workspace, uint64_t workspace_bytes, void* hip_stream);
/* Host arrays: SA and LCP go up into device buffers of the call's own on `device`, the results come down. lz77 is lpf followed by the
 * parse: an SA value >= n is CAPS_SA_EINVAL here too. */
int caps_sa_hip_lpf_u32(const uint32_t* SA, const uint32_t* LCP, uint64_t n, uint32_t* LPF, uint32_t* Prev, int device);
int caps_sa_hip_lpf_u64(const uint64_t* SA, const uint64_t* LCP, uint64_t n, uint64_t* LPF, uint64_t* Prev, int device);
int caps_sa_hip_lz77_u32(const uint32_t* SA, const uint32_t* LCP, uint64_t n, void* records, uint64_t capacity, uint64_t* n_phrases,
                         int device);
int caps_sa_hip_lz77_u64(const uint64_t* SA, const uint64_t* LCP, uint64_t n, void* records, uint64_t capacity, uint64_t* n_phrases,
                         int device);

/* ---- ISA and longest common extensions ---------------------------------------------
 * The inverse suffix array, and an index over (SA, LCP) that answers range minima over LCP and, from them, the longest common
 * extension of two text positions, exact or with up to k mismatches. n entries of width W (4 or 8 bytes); SA is a permutation of
 * 0 .. n - 1; LCP is any array, and LCP[0] counts as 0 whatever it holds.
 *   - ISA[SA[r]] = r.
 *   - range_min(lo, hi) = min LCP[lo .. hi] for RANKS lo <= hi < n, both ends inclusive, LCP[0] read as 0.
 *   - lce0(i, j) for positions i, j < n: n - i if i == j; otherwise min(range_min(min(a, b) + 1, max(a, b)), n - max(i, j)) with
 *     a = ISA[i], b = ISA[j]. For the arrays of a full-context build the clamp never bites; it keeps every read in range for any
 *     arrays. (Two equal ranks, which no permutation has, extend by 0.)
 *   - lce(i, j, k), 0 <= k <= 1024: the largest l <= n - max(i, j) such that T[i .. i + l) and T[j .. j + l) differ in at most k
 *     places, by kangaroo jumps: l = 0, used = 0; (2) l += lce0(i + l, j + l); stop if max(i, j) + l == n or used == k; otherwise
 *     l += 1, used += 1 and again from (2). At most k + 1 rounds.
 *
 * isa: dISA is n entries of the index width. A value SA[r] >= n is never used as an index; it, or a value that occurs twice (the
 * destination is preset to all ones and a slot still all ones afterwards is a position no rank names), is CAPS_SA_EINVAL ("not a
 * suffix array"). dISA is then unspecified (the host form leaves ISA as it was).
 *
 * The index is one relocatable blob, little-endian, every section rounded up to 256 bytes with zero padding (equal inputs give equal
 * blobs). B = 64 ranks per block, nb = ceil(n / 64); S = 4,096 ranks per superblock, ns = ceil(n / 4096); tl = 0 if n = 0, else
 * floor(log2 ns) + 1; up(b) = b rounded up to 256.
 *     offset                       bytes          content
 *     0                            256            header: 32 u64 words
 *                                                   0 magic "CAPSLCE1" (0x3145434C53504143)   1 version = 1     2 n
 *                                                   3 W (4 or 8)    4 B = 64    5 S = 4096    6 nb    7 ns    8 tl
 *                                                   9 off_isa    10 off_lcp    11 off_m    12 m_stride = up(nb W)
 *                                                   13 off_t     14 t_stride = up(ns W)    15 total    16 .. 31 zero
 *     off_isa = 256                up(n W)        ISA[n]
 *     off_lcp = off_isa + up(n W)  up(n W)        LCP[n], entry 0 stored as 0
 *     off_m = off_lcp + up(n W)    7 m_stride     M_0 .. M_6, nb entries each: M_j[b] = min LCP over the blocks
 *                                                 b .. min(b + 2^j, nb) - 1
 *     off_t = off_m + 7 m_stride   tl t_stride    T_0 .. T_{tl-1}, ns entries each: T_j[s] = min LCP over the superblocks
 *                                                 s .. min(s + 2^j, ns) - 1
 *     total = off_t + tl t_stride
 * caps_sa_hip_lce_index_bytes gives total: below 2 n W + n W / 8 + 16 KiB. The build needs no workspace beyond the blob, and the
 * blob alone answers queries: SA and LCP may be freed. Every header word follows from n and W: the query calls recompute all 32 on
 * the host and compare before a kernel reads the body; a blob with any other header, or longer than index_bytes, is CAPS_SA_EINVAL.
 * The body is not checked and need not be: for ANY body a range minimum makes at most 126 LCP reads and 6 table reads at addresses
 * that follow from (lo, hi) alone, a round of lce adds 2 ISA reads whose values are clamped to n - 1, and nothing walks a
 * data-dependent distance. A range minimum scans the partial blocks at its two ends (a block the range covers whole is taken from
 * M_0 instead), covers up to 64 whole blocks between them by two overlapping reads of M_j, j = floor(log2 count), and more than 64
 * by the blocks up to the next superblock edge (two reads of M_j), the whole superblocks (two reads of T_j) and the blocks from the
 * last edge (two reads of M_j).
 *
 * Queries: dLo, dHi, dI, dJ, dMin, dLen are u64[q]; the index width is read from the blob. A range with lo > hi or hi >= n, or a
 * position >= n, writes 0 to its slot and the call returns CAPS_SA_EINVAL after answering the others. Also CAPS_SA_EINVAL, checked
 * before any allocation, nothing written: a null pointer with n > 0 or q > 0, a null or not 16-byte aligned index, n > UINT32_MAX
 * with _u32, index_bytes below caps_sa_hip_lce_index_bytes (build) or below the blob (query), mismatches > 1024. n = 0 and q = 0
 * succeed. Device pointers are on the current device; the work runs on hip_stream and has completed on return. The host forms run
 * in the device block of the host-buffer builds; the blob a host build made, or the last one a host query uploaded, stays resident
 * there and is not uploaded again. Ranks beyond 2^32 (_u64 with n > UINT32_MAX) are untested: _u64 is tested at small sizes only.
 */
int caps_sa_hip_isa_device_u32(const void* dSA, uint64_t n, void* dISA, void* hip_stream);
int caps_sa_hip_isa_device_u64(const void* dSA, uint64_t n, void* dISA, void* hip_stream);
int caps_sa_hip_isa_u32(const uint32_t* SA, uint64_t n, uint32_t* ISA, int device);
int caps_sa_hip_isa_u64(const uint64_t* SA, uint64_t n, uint64_t* ISA, int device);
int caps_sa_hip_lce_index_bytes(uint64_t n, int idx_bytes, uint64_t* bytes);
int caps_sa_hip_lce_build_device_u32(const void* dSA, const void* dLCP, uint64_t n, void* dIndex, uint64_t index_bytes, void* hip_stream);
int caps_sa_hip_lce_build_device_u64(const void* dSA, const void* dLCP, uint64_t n, void* dIndex, uint64_t index_bytes, void* hip_stream);
int caps_sa_hip_lce_build_u32(const uint32_t* SA, const uint32_t* LCP, uint64_t n, void* index, uint64_t index_bytes, int device);
int caps_sa_hip_lce_build_u64(const uint64_t* SA, const uint64_t* LCP, uint64_t n, void* index, uint64_t index_bytes, int device);
int caps_sa_hip_lce_range_min_device(const void* dIndex, uint64_t index_bytes, const void* dLo, const void* dHi, uint64_t q, void* dMin,
                                     void* hip_stream);
int caps_sa_hip_lce_range_min(const void* index, uint64_t index_bytes, const uint64_t* lo, const uint64_t* hi, uint64_t q, uint64_t* min,
                              int device);
int caps_sa_hip_lce_device(const void* dIndex, uint64_t index_bytes, const void* dI, const void* dJ, uint64_t q, uint64_t mismatches,
                           void* dLen, void* hip_stream);
int caps_sa_hip_lce(const void* index, uint64_t index_bytes, const uint64_t* i, const uint64_t* j, uint64_t q, uint64_t mismatches,
                    uint64_t* len, int device);

/* ---- MUMs and MEMs between two texts ------------------------------------------------
 * The anchors a whole-sequence comparison starts from -- maximal unique matches (MUMs) and rare maximal exact matches (MEMs) between
 * A and B -- as rules over neighbouring ranks of the SA, LCP and BWT of T = A . sep . B. One streaming pass; the text is not read.
 *
 * Inputs: n entries of width W (4 or 8 bytes): SA, and LCP with LCP[0] counting as 0 whatever it holds. BWT: n bytes in rank order,
 * as caps_sa_hip_build_bwt_* / caps_sa_hip_bwt_device_* give them (BWT[r] = T[SA[r] - 1]; the byte at the rank with SA[r] == 0 is
 * never looked at). split in 0 .. n; side(p) = (p >= split): side 0 is A (with the separator), side 1 is B. The caller puts a byte
 * that occurs nowhere else at split - 1. Without one a match may run across the boundary; the result is then still exactly what the
 * rules below give on the arrays.
 *
 * LEFT-MAXIMAL: ranks p, q are left-maximal iff SA[p] == 0 or SA[q] == 0 or BWT[p] != BWT[q].
 *
 * MUM mode (cross_mums): rank r in 1 .. n - 1 yields a record iff, with l = LCP[r],
 *   1. l >= min_len;
 *   2. side(SA[r - 1]) != side(SA[r]);
 *   3. (r - 1 == 0 ? 0 : LCP[r - 1]) < l and (r + 1 < n ? LCP[r + 1] : 0) < l;
 *   4. r - 1 and r are left-maximal.
 *
 * MEM mode (cross_mems), max_occ in 2 .. CAPS_SA_CROSS_MAX_OCC:
 *   - A RUN is a maximal rank range [h, h') with LCP[i] >= min_len for every h < i < h' (the k-mer runs for k = min_len).
 *   - Runs with 2 <= h' - h <= max_occ are processed. Longer runs are skipped and counted, so the caller learns that the answer is
 *     partial.
 *   - In a processed run every pair p < q with different sides that is left-maximal yields a record with l = min LCP[p + 1 .. q].
 *   - This is every MEM of at least min_len bytes between A and B whose first min_len bytes occur at most max_occ times in T, each
 *     reported exactly once.
 *
 * Records: 24 bytes, little-endian:
 *     u64 a | u64 b | u64 len
 * a is the side-0 position and b the side-1 position, both absolute in T. MUM mode: in rank order. MEM mode: ordered by q ascending,
 * then p descending.
 *
 * summary (host, uint64_t[8]), always written: [0] the number of records; [1] the skipped runs (0 in MUM mode); [2..4] the longest
 * common substring: the maximum of LCP[r] over r in 1 .. n - 1 with side(SA[r - 1]) != side(SA[r]), independent of min_len and mode,
 * the lowest such r winning on ties -- its len, a and b, or 0, 0, 0 when there is none or the maximum is 0; [5..7] zero.
 *
 * Protocol and errors, as for caps_sa_hip_kmers*: dRecords = NULL is the counting call. A non-null dRecords (8-byte aligned) with
 * more records than capacity is CAPS_SA_EINVAL: the summary is still valid and no record is written. CAPS_SA_EINVAL, checked before
 * any allocation, with nothing written: min_len == 0; split > n; max_occ outside 2 .. 64 in MEM mode; a null array with n > 0; a
 * null summary; n > UINT32_MAX with _u32; a workspace that is too small. n = 0, split = 0 and split = n succeed with no records.
 *
 * For arrays that are no text's the calls terminate, read only [0, n) of each array and write only inside the outputs: nothing is
 * indexed by a value read from SA or LCP, and there is no validation pass. The work per rank is bounded for any input: in MEM mode a
 * rank reads at most max_occ + 1 entries of LCP and max_occ - 1 each of SA and BWT beside its own. A look-back or look-forward that
 * has not met a head within max_occ ranks gives the run up, consistently for every rank of it: 'A' * n with min_len = 1 is one run,
 * skipped, counted once (at its head). The workspace (caps_sa_hip_cross_workspace_bytes) is O(n / 16,384) words, no array of n
 * entries; NULL is allocated and freed by the call. dSA, dLCP, dBWT, dRecords and workspace are device pointers on the current
 * device; the work runs on hip_stream and has completed on return. Ranks beyond 2^32 (_u64 with n > UINT32_MAX) are untested.
 */
#define CAPS_SA_CROSS_MAX_OCC 64
int caps_sa_hip_cross_workspace_bytes(uint64_t n, int idx_bytes, uint64_t* bytes);
int caps_sa_hip_cross_mums_device_u32(const void* dSA, const void* dLCP, const void* dBWT, uint64_t n, uint64_t split, uint64_t min_len,
                                      void* dRecords, uint64_t capacity, uint64_t* summary, void* workspace, uint64_t workspace_bytes,
                                      void* hip_stream);
int caps_sa_hip_cross_mums_device_u64(const void* dSA, const void* dLCP, const void* dBWT, uint64_t n, uint64_t split, uint64_t min_len,
                                      void* dRecords, uint64_t capacity, uint64_t* summary, void* workspace, uint64_t workspace_bytes,
                                      void* hip_stream);
int caps_sa_hip_cross_mems_device_u32(const void* dSA, const void* dLCP, const void* dBWT, uint64_t n, uint64_t split, uint64_t min_len,
                                      uint32_t max_occ, void* dRecords, uint64_t capacity, uint64_t* summary, void* workspace,
                                      uint64_t workspace_bytes, void* hip_stream);
int caps_sa_hip_cross_mems_device_u64(const void* dSA, const void* dLCP, const void* dBWT, uint64_t n, uint64_t split, uint64_t min_len,
                                      uint32_t max_occ, void* dRecords, uint64_t capacity, uint64_t* summary, void* workspace,
                                      uint64_t workspace_bytes, void* hip_stream);
/* Host SA, LCP and BWT (and host records): the arrays go up into device buffers of the call's own on `device`, the records come down. */
int caps_sa_hip_cross_mums_u32(const uint32_t* SA, const uint32_t* LCP, const uint8_t* BWT, uint64_t n, uint64_t split, uint64_t min_len,
                               void* records, uint64_t capacity, uint64_t* summary, int device);
int caps_sa_hip_cross_mums_u64(const uint64_t* SA, const uint64_t* LCP, const uint8_t* BWT, uint64_t n, uint64_t split, uint64_t min_len,
                               void* records, uint64_t capacity, uint64_t* summary, int device);
int caps_sa_hip_cross_mems_u32(const uint32_t* SA, const uint32_t* LCP, const uint8_t* BWT, uint64_t n, uint64_t split, uint64_t min_len,
                               uint32_t max_occ, void* records, uint64_t capacity, uint64_t* summary, int device);
int caps_sa_hip_cross_mems_u64(const uint64_t* SA, const uint64_t* LCP, const uint8_t* BWT, uint64_t n, uint64_t split, uint64_t min_len,
                               uint32_t max_occ, void* records, uint64_t capacity, uint64_t* summary, int device);

/* ---- k-mers across a collection ------------------------------------------------------
 * Which k-mers the sequences of a collection share, from the SA and LCP of the text that holds them all: the text is not read.
 *
 * DOCUMENTS. m in 1 .. 64 and two host arrays doc_start[m], doc_len[m]: document d is T[doc_start[d] .. doc_start[d] + doc_len[d]).
 * The ranges are ascending and disjoint -- doc_start[d] + doc_len[d] <= doc_start[d + 1], the last one ends at or before n, all of it
 * computed without overflow. Gaps belong to no document (separators, headers, nothing). A length of 0 is allowed.
 *
 * RUNS. Heads and runs are those of "k-mers from SA and LCP": rank i is a head iff i == 0 or LCP[i] < k; LCP[0] counts as 0.
 *
 * RANKS. Rank r with p = SA[r] is IN document d iff doc_start[d] <= p and p + k <= doc_start[d] + doc_len[d], computed without
 * overflow; otherwise it is OUT: a position in a gap, a k-mer that runs past its document's end, p >= n in arrays that are no text's.
 * Of a run:  docs = the OR of 1 << d over its IN ranks,  occ = the number of its IN ranks,  count = its length in ranks.
 * A run is a COLLECTION K-MER iff docs != 0; its bytes are T[SA[first] .. SA[first] + k).
 * Where documents touch without a separator a run may mix IN and OUT ranks (the k-mer also occurs across a boundary): the rule above
 * is then the definition, count > occ. With a separator byte that occurs in no document every run is all IN or all OUT.
 *
 * coll_kmers: the collection k-mers in rank order (the library's byte order) as records of 32 bytes, little-endian:
 *     u64 first | u64 count | u64 occ | u64 docs
 * A record is written iff, with c = popcount(docs): min_docs <= c (min_docs = 0 is treated as 1), c <= max_docs unless max_docs == 0,
 * (docs & all_of) == all_of and (docs & none_of) == 0. min_docs > m is no error: no record.
 * The protocol of caps_sa_hip_kmers*: dRecords = NULL is the counting call; *n_records (host) is always written by a call that is not
 * refused; a non-null dRecords (8-byte aligned) with *n_records > capacity is CAPS_SA_EINVAL, *n_records still valid, nothing written.
 *
 * coll_sharing: the summary of every collection k-mer, unfiltered.
 *     freq (host, u64[65]):  freq[c] = the collection k-mers with popcount(docs) == c; freq[0] = 0 (all 65 words are written).
 *     shared (host, u64[m * m], row-major):  shared[a * m + b] = the collection k-mers whose docs has both bit a and bit b. The
 *     diagonal is the number of distinct k-mers of document a, the matrix is symmetric, and
 *     Jaccard(a, b) = S_ab / (S_aa + S_bb - S_ab), containment of a in b = S_ab / S_aa.
 *
 * CAPS_SA_EINVAL, checked before any allocation, nothing written: k == 0; m == 0 or m > 64; null document arrays; ranges that overlap,
 * descend or pass n; min_docs > max_docs > 0; all_of & none_of != 0; a mask bit at or above m; a null array with n > 0; a null output;
 * n > UINT32_MAX with _u32; a workspace that is too small. n = 0 succeeds with zeros.
 *
 * Arrays of a bounded-context build are not a suffix array: the result is then unspecified. For arrays that are not the SA / LCP of any
 * text the calls still terminate, read only SA[0 .. n) and LCP[0 .. n) and write only inside the outputs: no value read from the arrays
 * becomes an index -- the document of a position comes from a search over the at most 64 starts, which are compared, not indexed.
 * There is no validation pass. Ranks beyond 2^32 (_u64 with n > UINT32_MAX) are untested.
 *
 * The workspace (caps_sa_hip_coll_workspace_bytes) is O(n / 16,384) words and a fixed part of about 34 MB, no array of n entries; NULL is
 * allocated and freed by the call. dSA, dLCP, dRecords and workspace are device pointers on the current device; doc_start, doc_len,
 * freq, shared and n_records are host pointers; the work runs on hip_stream and has completed on return.
 */
int caps_sa_hip_coll_workspace_bytes(uint64_t n, int idx_bytes, uint64_t* bytes);
int caps_sa_hip_coll_kmers_device_u32(const void* dSA, const void* dLCP, uint64_t n, uint64_t k, const uint64_t* doc_start,
                                      const uint64_t* doc_len, uint32_t m, uint64_t min_docs, uint64_t max_docs, uint64_t all_of,
                                      uint64_t none_of, void* dRecords, uint64_t capacity, uint64_t* n_records, void* workspace,
                                      uint64_t workspace_bytes, void* hip_stream);
int caps_sa_hip_coll_kmers_device_u64(const void* dSA, const void* dLCP, uint64_t n, uint64_t k, const uint64_t* doc_start,
                                      const uint64_t* doc_len, uint32_t m, uint64_t min_docs, uint64_t max_docs, uint64_t all_of,
                                      uint64_t none_of, void* dRecords, uint64_t capacity, uint64_t* n_records, void* workspace,
                                      uint64_t workspace_bytes, void* hip_stream);
int caps_sa_hip_coll_sharing_device_u32(const void* dSA, const void* dLCP, uint64_t n, uint64_t k, const uint64_t* doc_start,
                                        const uint64_t* doc_len, uint32_t m, uint64_t* freq, uint64_t* shared, void* workspace,
                                        uint64_t workspace_bytes, void* hip_stream);
int caps_sa_hip_coll_sharing_device_u64(const void* dSA, const void* dLCP, uint64_t n, uint64_t k, const uint64_t* doc_start,
                                        const uint64_t* doc_len, uint32_t m, uint64_t* freq, uint64_t* shared, void* workspace,
                                        uint64_t workspace_bytes, void* hip_stream);
/* Host SA and LCP (and host records): the arrays go up into device buffers of the call's own on `device`, the records come down. */
int caps_sa_hip_coll_kmers_u32(const uint32_t* SA, const uint32_t* LCP, uint64_t n, uint64_t k, const uint64_t* doc_start,
                               const uint64_t* doc_len, uint32_t m, uint64_t min_docs, uint64_t max_docs, uint64_t all_of, uint64_t none_of,
                               void* records, uint64_t capacity, uint64_t* n_records, int device);
int caps_sa_hip_coll_kmers_u64(const uint64_t* SA, const uint64_t* LCP, uint64_t n, uint64_t k, const uint64_t* doc_start,
                               const uint64_t* doc_len, uint32_t m, uint64_t min_docs, uint64_t max_docs, uint64_t all_of, uint64_t none_of,
                               void* records, uint64_t capacity, uint64_t* n_records, int device);
int caps_sa_hip_coll_sharing_u32(const uint32_t* SA, const uint32_t* LCP, uint64_t n, uint64_t k, const uint64_t* doc_start,
                                 const uint64_t* doc_len, uint32_t m, uint64_t* freq, uint64_t* shared, int device);
int caps_sa_hip_coll_sharing_u64(const uint64_t* SA, const uint64_t* LCP, uint64_t n, uint64_t k, const uint64_t* doc_start,
                                 const uint64_t* doc_len, uint32_t m, uint64_t* freq, uint64_t* shared, int device);

/* ---- kernel-level entry points (host buffers) for differential tests -------------- */

/* merge_sort (src/Suffix_Array.cpp:112-129) of an arbitrary list of cnt distinct suffix
 * positions: out_sa = sorted list, out_lcp = its LCP array (out_lcp[0] = 0). */
int caps_sa_hip_sort_suffixes_u32(const char* T, uint64_t n, const uint32_t* idx, uint64_t cnt,
                                  uint32_t* out_sa, uint32_t* out_lcp, int device);
int caps_sa_hip_sort_suffixes_u64(const char* T, uint64_t n, const uint64_t* idx, uint64_t cnt,
                                  uint64_t* out_sa, uint64_t* out_lcp, int device);

/* sort_partition over every partition (src/Suffix_Array.cpp:388-404): independent sorts of
 * the G consecutive segments [seg_start[g], seg_start[g+1]) of the suffix list idx (seg_start:
 * host u64[G+1], seg_start[0] = 0, seg_start[G] = cnt).  out_lcp at a segment head is the lcp
 * with the last suffix of the previous non-empty segment (cpp:431-447); out_lcp[0] = 0. */
int caps_sa_hip_sort_segments_u32(const char* T, uint64_t n, const uint32_t* idx, uint64_t cnt,
                                  const uint64_t* seg_start, uint64_t G, uint32_t* out_sa, uint32_t* out_lcp, int device);
int caps_sa_hip_sort_segments_u64(const char* T, uint64_t n, const uint64_t* idx, uint64_t cnt,
                                  const uint64_t* seg_start, uint64_t G, uint64_t* out_sa, uint64_t* out_lcp, int device);

/* merge (src/Suffix_Array.cpp:48-109): X, Y sorted suffix runs with their LCP arrays ->
 * Z (len_x + len_y) and LCP_z. */
int caps_sa_hip_merge_u32(const char* T, uint64_t n, const uint32_t* X, uint64_t len_x, const uint32_t* Y,
                          uint64_t len_y, const uint32_t* LCP_x, const uint32_t* LCP_y, uint32_t* Z,
                          uint32_t* LCP_z, int device);   /* LCP_x/LCP_y: accepted, not needed (keys) */
int caps_sa_hip_merge_u64(const char* T, uint64_t n, const uint64_t* X, uint64_t len_x, const uint64_t* Y,
                          uint64_t len_y, const uint64_t* LCP_x, const uint64_t* LCP_y, uint64_t* Z,
                          uint64_t* LCP_z, int device);

/* upper_bound (src/Suffix_Array.cpp:252-297) without the 65,536-char cutoff: for each
 * pivot suffix position, the number of elements of the sorted list X that are <= it. */
int caps_sa_hip_upper_bound_u32(const char* T, uint64_t n, const uint32_t* X, uint64_t cnt,
                                const uint32_t* pivots, uint64_t n_pivots, uint32_t* out, int device);
int caps_sa_hip_upper_bound_u64(const char* T, uint64_t n, const uint64_t* X, uint64_t cnt,
                                const uint64_t* pivots, uint64_t n_pivots, uint64_t* out, int device);

/* LCP<8> (include/Suffix_Array.hpp:195-241): out[i] = lcp(T[a[i]..), T[b[i]..)). */
int caps_sa_hip_lcp_u32(const char* T, uint64_t n, const uint32_t* a, const uint32_t* b, uint64_t cnt,
                        uint32_t* out, int device);
int caps_sa_hip_lcp_u64(const char* T, uint64_t n, const uint64_t* a, const uint64_t* b, uint64_t cnt,
                        uint64_t* out, int device);


/* ---- multi-GPU: one shard per process/GPU ----------------------------
 * The reference has no distributed mode; these entry points cut construct() at its one
 * exchange step (partition_sub_subarrays, src/Suffix_Array.cpp:300-368) so that a host
 * driver can run the collectives between them (caps_sa_dist.py: torch.distributed / RCCL):
 *
 *   shard_create -> shard_phase1 -> [all_gather samples] -> shard_pivots
 *   -> [all_gather partition sizes] -> shard_collate -> [all_to_all_v of (key, sa)]
 *   -> shard_phase2 -> [all_gather last SA] -> shard_fix_first_lcp
 *
 * The text is replicated (dT: n bytes on this rank's device).  Rank r sorts subarrays
 * [r*p/world, (r+1)*p/world) and ends up owning a contiguous slice of the global SA/LCP.
 * All d_* pointers are device pointers on the rank's device; idx_bytes is 4 or 8. */
typedef struct caps_sa_shard caps_sa_shard;
typedef struct caps_sa_shard_info {
    uint64_t n;
    uint32_t p, ppp, rank, world;
    uint32_t g0, g1;               /* subarrays sorted by this rank */
    uint32_t bits_per_char, idx_bytes;
    uint32_t part_lo, part_hi;     /* partitions owned after shard_collate */
    uint64_t local_elems;          /* elements of this rank's subarrays = capacity of the send buffers */
    uint64_t m_local, m_total;     /* samples of this rank / of all ranks */
    uint64_t recv_total;           /* elements of the owned partitions (after shard_collate) */
    uint64_t slice_off;            /* position of the rank's slice in the global SA/LCP */
    uint64_t capacity;             /* most elements this shard can receive (size of recv / SA / LCP buffers) */
    double ms_phase1, ms_pivots, ms_collate, ms_phase2;
    /* direct path (shard_scatter / shard_plan / shard_sort) */
    uint32_t direct_fallback;      /* CAPS_SA_FB_NONE: the shape allows the direct path; else why not */
    uint32_t direct_groups, direct_sub, n_streams;   /* groups, sub-streams per group, streams = groups x sub-streams */
    uint64_t stream_cap;           /* elements a stream region holds */
    uint64_t send_capacity;        /* elements the send buffers must hold (either path) */
    double ms_scatter, ms_sort;
    /* kernel families of the last direct build on this rank (HIP events on its stream) */
    double ms_level_a, ms_level_b, ms_tile_sort, ms_merge_passes;
    uint64_t level_a_elems;        /* text positions this rank distributed */
    uint32_t slot_splits, slot_splits_redone;
    uint32_t key_bytes;            /* bytes per key in the send / receive buffers of the last shard_scatter: 8, or 4 (32-bit keys,
                                      csrc/text.h key32_of: what travels when world > 1 on 2-bit texts) */
    uint32_t exchange;             /* 1: the streams shard_scatter wrote must be exchanged (all-to-all by the counts of shard_plan)
                                      before shard_sort; 0 (the default for the direct path): nothing travels -- every rank
                                      scattered the whole text and kept its own groups; shard_sort reads the send buffers */
    uint32_t direct_quantile;      /* 1: the last shard_scatter chose quantile buckets for level B (skewed keys, frequent keys, long
                                      runs; csrc/pipeline.h Builder::run_direct) -- no-exchange mode only */
    uint32_t run_buckets;          /* letter-run buckets of the last shard_sort (see caps_sa_stats.run_buckets) */
    uint64_t tie_groups_deferred;  /* groups of equal keys the last shard_sort re-keyed instead of comparing (see caps_sa_stats; no-exchange
                                      mode, 64-bit keys) */
    uint32_t tie_levels, reserved_;
} caps_sa_shard_info;

int caps_sa_hip_shard_create(const void* dT, uint64_t n, uint64_t subproblem_count, int idx_bytes, int rank, int world,
                             void* hip_stream, caps_sa_shard** out);
void caps_sa_hip_shard_destroy(caps_sa_shard* s);
int caps_sa_hip_shard_info(const caps_sa_shard* s, caps_sa_shard_info* info);
/* d_sample_keys: u64[m_local], d_sample_sa: idx[m_local] */
int caps_sa_hip_shard_phase1(caps_sa_shard* s, void* d_sample_keys, void* d_sample_sa);
/* d_all_keys: u64[m_total], d_all_sa: idx[m_total] (any order); d_local_sizes: u64[p] out */
int caps_sa_hip_shard_pivots(caps_sa_shard* s, const void* d_all_keys, const void* d_all_sa, void* d_local_sizes);
/* all_sizes: HOST u64[world][p]; d_send_*: [local_elems]; send_counts/recv_counts: HOST u64[world] out */
int caps_sa_hip_shard_collate(caps_sa_shard* s, const uint64_t* all_sizes, void* d_send_keys, void* d_send_sa,
                              uint64_t* send_counts, uint64_t* recv_counts);
/* d_recv_*: [recv_total], source-rank-major; dSA/dLCP: idx[recv_total] out */
int caps_sa_hip_shard_phase2(caps_sa_shard* s, const void* d_recv_keys, const void* d_recv_sa, void* dSA, void* dLCP);
/*
 * Direct path of a sharded build (what Builder::run_direct does on one GPU; no sort_subarrays, no locate_pivots):
 *
 *   shard_create -> shard_scatter -> [all_gather of the reports] -> shard_plan
 *   -> [only if shard_info.exchange: all-to-all of the (key, sa) blocks] -> shard_sort -> [all_gather last SA] -> shard_fix_first_lcp
 *
 * shard_scatter: packs the text, derives the pivots (every rank the same ones, from the same samples of the text) and
 * distributes suffixes into stream regions of d_send_keys (u64[send_capacity]) / d_send_sa (idx[send_capacity]).
 *   Default (shard_info.exchange = 0): the suffixes of the WHOLE text that belong to the groups this rank owns -- the text is
 *   replicated, so no element has to cross a link; shard_plan then returns all-zero counts and shard_sort reads the send
 *   buffers (d_recv_* = d_send_*).
 *   CAPS_SA_SHARD_EXCHANGE=1 (exchange = 1): the suffixes of every world-th tile of the text, all groups; the block for rank d
 *   is contiguous, shard_plan returns the elements to send to / receive from every rank (gaps of the regions included) and
 *   shard_sort takes the received blocks in rank order.
 * d_report: u64[n_streams + 2], this rank's stream sizes and flags.  shard_plan: all_reports = HOST u64[world][n_streams + 2];
 * returns 0, or a positive CAPS_SA_FB_* code -- the same on every rank -- when the text cannot be split by keys alone: the
 * ranks then run the samplesort sequence above (shard_phase1 ...).  shard_sort: dSA / dLCP: idx[capacity] out, recv_total
 * entries valid.  When d_recv_* ARE the send buffers of the last shard_scatter (exchange = 0), shard_sort may rewrite them: large
 * groups of equal keys are then re-keyed instead of compared, and if that refinement does not fit its work memory the shard
 * scatters into the same buffers once more and sorts with every tie compared.  Buffers of the caller's own are read only.
 */
int caps_sa_hip_shard_scatter(caps_sa_shard* s, void* d_send_keys, void* d_send_sa, void* d_report);
int caps_sa_hip_shard_plan(caps_sa_shard* s, const uint64_t* all_reports, uint64_t* send_counts, uint64_t* recv_counts);
int caps_sa_hip_shard_sort(caps_sa_shard* s, const void* d_recv_keys, const void* d_recv_sa, void* dSA, void* dLCP);
/* Key width (exchange = 1 only): shard_scatter writes 32-bit keys (shard_info.key_bytes = 4: d_send_keys / d_recv_keys are then u32
 * arrays) when the world has more than one rank and the text packs to 2 bits -- a third fewer bytes cross xGMI.  shard_sort then returns
 * CAPS_SA_FB_KEY32 (> 0) when a bucket slot overflowed (skewed keys the pivots did not reveal); the ranks take the maximum
 * of their codes, and if it is not 0 every rank calls shard_set_key_bits(s, 64) and repeats scatter / exchange / sort. */
int caps_sa_hip_shard_set_key_bits(caps_sa_shard* s, int bits);
/* Differential tests: copies this rank's sorted subarrays after shard_phase1 into d_keys_out (u64[count]) / d_sa_out
 * (idx[count]) (either may be NULL: sizes only); subarray g of the rank = entries [g * subarray_len, (g + 1) * subarray_len),
 * the last one to the end. */
int caps_sa_hip_shard_phase1_arrays(caps_sa_shard* s, void* d_keys_out, void* d_sa_out, uint64_t* count, uint64_t* subarray_len);
/* last SA value of the slice (UINT64_MAX when the slice is empty) */
int caps_sa_hip_shard_last_sa(caps_sa_shard* s, uint64_t* last_sa);
/* prev_sa: last SA value of the nearest non-empty lower rank (UINT64_MAX: none) */
int caps_sa_hip_shard_fix_first_lcp(caps_sa_shard* s, uint64_t prev_sa, void* dLCP);

#ifdef __cplusplus
}
#endif
#endif /* CAPS_SA_HIP_H */
