// caps-sa_amd/csrc/kernels.h
//
// The HIP kernels of the suffix-array / LCP-array construction path, written for
// gfx950 (CDNA4, wave64, 160 KiB LDS per CU) in the phase style of kernel_lang.h.
//
// Reference rows -> kernels:
//   a2 LCP<8> comparator                      -> text.h (window64 / pair_lcp / suffix_less)
//   a4 merge_sort, a5 sort_subarrays          -> tile_sort_kernel (+ merge passes below)
//   a3 merge (LCP-merge of two runs)          -> merge_partition_kernel + merge_pass_kernel
//   a6 sample_pivots / select_pivots          -> sample_kernel, pick_pivots_kernel (+ the sorts)
//   a7 upper_bound, a8 locate_pivots          -> locate_kernel
//   a9 partition_sub_subarrays                -> partition_sizes_kernel, scan_sizes_kernel,
//                                                collate_kernel
//   a10 merge_sub_subarrays / sort_partition  -> tile_sort_kernel + merge passes per partition
//   a11 compute_partition_boundary_lcp        -> finalize_kernel (segment-head LCPs while gathering SA/LCP)
//
// Data layout in HBM: struct-of-arrays per element -- key (u64, first 64/BITS chars of
// the suffix), sa (idx_t, text position), and -- written only by the sort step that
// completes a segment -- lcp (idx_t, lcp with the predecessor in the sorted segment; 0 for
// the segment head, the reference's convention at src/Suffix_Array.cpp:117-118,354-356).  A "segment" is an independent sort problem
// (a subarray in phase 1, the sample set, a partition in phase 2); segments are
// described by seg_start[G+1] and are cut into tiles of TILE_E elements aligned to the
// segment start.
#pragma once
#include "kernel_lang.h"
#include "text.h"

namespace caps {

// Tile geometry (compile-time; -DCAPS_TILE_E=... etc. build the variants compared in
// profiles/).  Default: 4096-element tiles, 1024 threads, two workgroups per CU
// (LDS 48 KiB at 32-bit indices, 64 KiB at 64-bit; 8 waves per SIMD => 64 VGPRs).
#ifndef CAPS_TILE_E
#define CAPS_TILE_E 4096
#endif
#ifndef CAPS_TILE_NT
#define CAPS_TILE_NT 1024
#endif
#ifndef CAPS_TILE_WAVES
#define CAPS_TILE_WAVES 8          /* min waves per SIMD = workgroups per CU * CAPS_TILE_NT / 256 */
#endif
#ifndef CAPS_LOCK_K
#define CAPS_LOCK_K 4              /* binary searches one thread advances in lockstep */
#endif
constexpr uint32_t TILE_E = CAPS_TILE_E;       // elements per tile (one workgroup)
constexpr uint32_t TILE_NT = CAPS_TILE_NT;     // threads per tile workgroup
constexpr uint32_t TILE_EPT = TILE_E / TILE_NT;
constexpr uint32_t LOCK_K = CAPS_LOCK_K < TILE_EPT ? CAPS_LOCK_K : TILE_EPT;
#define TILE_WAVES_PER_SIMD CAPS_TILE_WAVES
#ifdef CAPS_NO_WAVES_BOUND   /* experiment: let the compiler pick the register budget */
#undef LAUNCH_BOUNDS2
#define LAUNCH_BOUNDS2(n, w) LAUNCH_BOUNDS(n)
#endif
static_assert(TILE_E % TILE_NT == 0 && TILE_EPT % LOCK_K == 0, "tile geometry");
#ifndef CAPS_TILE_BINS_DIV
#define CAPS_TILE_BINS_DIV 2
#endif
constexpr uint32_t TILE_BINS_ = TILE_E / CAPS_TILE_BINS_DIV;   // bins of the in-LDS bucket sort of one tile

// Segment/tile descriptor shared by the tile-granular kernels.
// One record per tile, written once by tile_map_kernel: a tile kernel starts with ONE load of
// its record instead of the dependent chain tile -> segment -> segment bounds (a workgroup is
// a few microseconds of work, so every dependent global load at its start shows).
struct alignas(16) TileInfo {
    uint64_t s0, s1;     // segment range
    uint32_t tl;         // tile index inside the segment
    uint32_t g;          // segment
    uint32_t pad_[2];
};

struct SegDesc {
    const uint64_t* seg_start;   // [G+1] element offsets of the segments
    const uint32_t* tile_off;    // [G+1] exclusive scan of ceil(len/TILE_E); tile_off[G] = #tiles
    const TileInfo* tile_rec;    // [#tiles] record of each tile
    uint32_t G;
};

// End of segment g: seg_start[g + 1] for contiguous segments; seg_end[g] when the segments sit in
// fixed-capacity regions with gaps between them (the groups of the direct path, pipeline.h).
DEV_INLINE uint64_t seg_end_of(const uint64_t* __restrict__ seg_start, const uint64_t* __restrict__ seg_end, uint64_t g)
{
    return seg_end ? seg_end[g] : seg_start[g + 1];
}

DEV_INLINE TileInfo tile_info(const SegDesc& sd, uint32_t b) { return sd.tile_rec[b]; }

// Geometry of the run pair a tile belongs to during a merge pass with run length R
// (R is a multiple of TILE_E).  single_la != ~0: the segment is ONE pair whose first run
// has length single_la (used by the stand-alone merge entry point).
struct PairInfo {
    uint64_t a0;         // start of run A (= start of the merged output)
    uint64_t la, lb;     // run lengths
    uint64_t d0;         // first output diagonal of this tile inside the pair
};

DEV_INLINE PairInfo pair_info(const TileInfo& t, uint64_t R, uint64_t single_la)
{
    PairInfo p;
    if (single_la != ~0ull) {
        p.a0 = t.s0;
        p.la = single_la;
        p.lb = (t.s1 - t.s0) - single_la;
        p.d0 = (uint64_t)t.tl * TILE_E;
        return p;
    }
    const uint64_t tpp = (2 * R) / TILE_E;             // tiles per pair
    const uint64_t q = t.tl / tpp;
    p.a0 = t.s0 + q * 2 * R;
    const uint64_t left = t.s1 - p.a0;
    p.la = left < R ? left : R;
    p.lb = left - p.la < R ? left - p.la : R;
    p.d0 = ((uint64_t)t.tl - q * tpp) * TILE_E;
    return p;
}

// ----------------------------------------------------------------------------------
// Input preparation
// ----------------------------------------------------------------------------------

// Which byte values occur in T: 256-bit presence set (8 x u32), OR-reduced.
// 16 bytes per lane per load; a byte marks its flag in a 256-entry LDS table with a plain
// store (idempotent, so colliding lanes need no atomic); the table is folded into the global
// bit set once per workgroup.  T must be readable in 16-byte units up to n rounded up (the
// callers' buffers are; the tail is handled bytewise).
GLOBAL_FN LAUNCH_BOUNDS(256) alphabet_kernel(KCTX const uint8_t* __restrict__ T, uint64_t n, uint32_t* __restrict__ present)
{
    SHARED_ARRAY(uint32_t, flags, 256);
    PAR(tid) { flags[tid & 255] = 0; }
    SYNC();
    PAR(tid) {
        const uint64_t stride = (uint64_t)K_GRID_DIM * K_BLOCK_DIM * 16;
        const bool aligned = (reinterpret_cast<uintptr_t>(T) & 15) == 0;
        for (uint64_t i = ((uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid) * 16; i < n; i += stride) {
            if (aligned && i + 16 <= n) {
                const uint32_t* q = reinterpret_cast<const uint32_t*>(T + i);
                const uint32_t w[4] = {q[0], q[1], q[2], q[3]};
                UNROLL
                for (int k = 0; k < 4; ++k) {
                    flags[w[k] & 255] = 1;
                    flags[(w[k] >> 8) & 255] = 1;
                    flags[(w[k] >> 16) & 255] = 1;
                    flags[w[k] >> 24] = 1;
                }
            } else {
                const uint64_t e = i + 16 < n ? i + 16 : n;
                for (uint64_t j = i; j < e; ++j) flags[T[j]] = 1;
            }
        }
    }
    SYNC();
    PAR(tid) {
        if (tid < 256 && flags[tid]) ATOMIC_OR_U32(&present[tid >> 5], 1u << (tid & 31));
    }
}

// Pack raw bytes into BITS-wide codes, big-endian inside each 32-bit word (text.h).
// lut[256] maps byte -> code (staged in LDS).  One thread per 16 input bytes (one 16-byte
// load -> one word at BITS = 2, four words at BITS = 8); words past the text are 0.
// bad != null: the LUT comes from a SAMPLE of the text (prepare_text); a byte it does not know (code 0xFF) raises bad[0] and
// the caller redoes the preparation with the alphabet of the whole text.
template <int BITS>
GLOBAL_FN LAUNCH_BOUNDS(256) pack_kernel(KCTX const uint8_t* __restrict__ T, uint64_t n, const uint8_t* __restrict__ lut,
                                         uint32_t* __restrict__ P, uint64_t n_words, uint32_t* __restrict__ bad)
{
    constexpr uint32_t CPW = TextTraits<BITS>::CPW;
    constexpr uint32_t WPT = 16 / CPW;                    // output words per 16 input bytes
    SHARED_ARRAY(uint8_t, slut, 256);
    PAR(tid) { slut[tid & 255] = lut[tid & 255]; }
    SYNC();
    PAR(tid) {
        const uint64_t stride = (uint64_t)K_GRID_DIM * K_BLOCK_DIM;
        const uint64_t n_units = (n_words + WPT - 1) / WPT;
        const bool aligned = (reinterpret_cast<uintptr_t>(T) & 15) == 0;
        for (uint64_t u = (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid; u < n_units; u += stride) {
            const uint64_t base = u * 16;
            uint8_t c[16];
            if (aligned && base + 16 <= n) {
                const uint32_t* q = reinterpret_cast<const uint32_t*>(T + base);
                UNROLL
                for (int k = 0; k < 4; ++k) {
                    const uint32_t w = q[k];
                    c[4 * k] = (uint8_t)w; c[4 * k + 1] = (uint8_t)(w >> 8); c[4 * k + 2] = (uint8_t)(w >> 16); c[4 * k + 3] = (uint8_t)(w >> 24);
                }
            } else {
                UNROLL
                for (int k = 0; k < 16; ++k) c[k] = base + k < n ? T[base + k] : 0;
            }
            uint32_t unknown = 0;
            UNROLL
            for (uint32_t wo = 0; wo < WPT; ++wo) {
                uint32_t v = 0;
                UNROLL
                for (uint32_t k = 0; k < CPW; ++k) {
                    const uint64_t i = base + wo * CPW + k;
                    const uint32_t code = i < n ? slut[c[wo * CPW + k]] : 0u;
                    unknown |= code;
                    v |= (code & ((1u << BITS) - 1u)) << (32 - BITS * (k + 1));
                }
                if (u * WPT + wo < n_words) P[u * WPT + wo] = v;
            }
            if (BITS == 2 && bad && (unknown & 0x80u)) bad[0] = 1;       // benign race: every writer stores 1
        }
    }
}

// Run table (text.h), step 1: one entry per aligned block of KCH chars.  A block with smallest
// period d whose d-periodic stretch ends inside the next block (or at the end of the text) gets
// its final value; one whose stretch covers the whole next block gets RUN_LINKED (= "the value
// of the block after me": that block then has the same smallest period) and raises *flag.
// Blocks that are aperiodic or reach past the text get 0.
template <int BITS>
GLOBAL_FN LAUNCH_BOUNDS(256) run_blocks_kernel(KCTX const uint32_t* __restrict__ P, uint64_t n, uint64_t entries,
                                               uint64_t* __restrict__ R, uint64_t* __restrict__ flag)
{
    constexpr uint32_t KCH = TextTraits<BITS>::KCH;
    PAR(tid) {
        const uint64_t full = n / KCH;                            // blocks that lie inside the text
        const uint64_t stride = (uint64_t)K_GRID_DIM * K_BLOCK_DIM;
        bool linked = false;
        for (uint64_t b = (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid; b < entries; b += stride) {
            uint64_t r = 0;
            if (b < full) {
                const uint64_t w0 = ((uint64_t)P[2 * b] << 32) | P[2 * b + 1];
                const uint32_t d = block_period<BITS>(w0);
                if (d) {
                    const uint64_t w1 = ((uint64_t)P[2 * b + 2] << 32) | P[2 * b + 3];
                    const uint32_t sh = d * BITS;
                    const uint64_t x = w1 ^ ((w0 << (64 - sh)) | (w1 >> sh));   // T[q] ^ T[q - d] over the next block
                    const uint64_t cand = x ? KCH * (b + 1) + (uint32_t)caps_clz64(x) / BITS : KCH * (b + 2);
                    if (cand >= n) r = ((uint64_t)d << 56) | n;
                    else if (!x) { r = RUN_LINKED; linked = true; }
                    else r = ((uint64_t)d << 56) | cand;
                }
            }
            R[b] = r;
        }
        if (linked) *flag = 1;                                     // benign race: every writer stores 1
    }
}

// Run table, steps 2-4: R[b] = R[first block >= b that is not RUN_LINKED], a suffix scan with the
// operator "mine unless linked".  Chunks of RUN_CHUNK blocks: (2) first unlinked value of every
// chunk, (3) one workgroup carries them from the right, (4) every chunk resolves its entries.
// All three return at once when no block is linked (any text without a periodic stretch of
// 2 * KCH chars: step 1 has already written final values).
GLOBAL_FN LAUNCH_BOUNDS(256) run_chunk_heads_kernel(KCTX const uint64_t* __restrict__ R, uint64_t entries,
                                                    const uint64_t* __restrict__ flag, uint64_t* __restrict__ head)
{
    SHARED_ARRAY(uint32_t, first, 1);
    if (!*flag) return;
    PAR(tid) { if (tid == 0) first[0] = RUN_CHUNK; }
    SYNC();
    const uint64_t base = (uint64_t)K_BLOCK_IDX * RUN_CHUNK;
    PAR(tid) {
        for (uint32_t k = 0; k < RUN_PER; ++k) {
            const uint64_t b = base + (uint64_t)tid * RUN_PER + k;
            if (b < entries && R[b] != RUN_LINKED) {
                ATOMIC_MIN_U32(&first[0], tid * RUN_PER + k);
                break;
            }
        }
    }
    SYNC();
    PAR(tid) {
        if (tid == 0) head[K_BLOCK_IDX] = first[0] < RUN_CHUNK ? R[base + first[0]] : RUN_LINKED;
    }
}

// carry[c] = first unlinked value right of chunk c (exclusive); one workgroup, right to left.
GLOBAL_FN LAUNCH_BOUNDS(1024) run_carry_kernel(KCTX const uint64_t* __restrict__ head, uint32_t chunks,
                                               const uint64_t* __restrict__ flag, uint64_t* __restrict__ carry)
{
    SHARED_ARRAY(uint64_t, v, 2 * 1024);
    SHARED_ARRAY(uint64_t, from_right, 1);
    if (!*flag) return;
    PAR(tid) { if (tid == 0) from_right[0] = 0; }              // the last entries of the table are 0, never linked
    SYNC();
    for (uint64_t hi = chunks; hi > 0; hi -= (hi < 1024 ? hi : 1024)) {
        const uint32_t cnt = (uint32_t)(hi < 1024 ? hi : 1024);
        const uint64_t lo = hi - cnt;                              // this round: chunks [lo, hi)
        PAR(tid) { v[tid] = tid < cnt ? head[lo + tid] : RUN_LINKED; }
        SYNC();
        uint32_t src = 0;
        for (uint32_t d = 1; d < 1024; d <<= 1) {                  // inclusive suffix scan, ping-pong halves
            PAR(tid) {
                const uint64_t mine = v[src * 1024 + tid];
                v[(src ^ 1) * 1024 + tid] = (mine == RUN_LINKED && tid + d < 1024) ? v[src * 1024 + tid + d] : mine;
            }
            SYNC();
            src ^= 1;
        }
        PAR(tid) {
            if (tid < cnt) {
                const uint64_t right = tid + 1 < cnt ? v[src * 1024 + tid + 1] : RUN_LINKED;   // inclusive value of the chunk to my right
                carry[lo + tid] = right != RUN_LINKED ? right : from_right[0];
            }
        }
        SYNC();
        PAR(tid) {
            if (tid == 0 && v[src * 1024] != RUN_LINKED) from_right[0] = v[src * 1024];
        }
        SYNC();
    }
}

// Also: longest[0] = max over blocks of (end of its stretch - start of the block).
GLOBAL_FN LAUNCH_BOUNDS(256) run_resolve_kernel(KCTX uint64_t* __restrict__ R, uint64_t entries, const uint64_t* __restrict__ flag,
                                                const uint64_t* __restrict__ carry, uint32_t kch, uint64_t* __restrict__ longest)
{
    SHARED_ARRAY(uint64_t, v, 2 * RUN_NT);
    SHARED_ARRAY(uint64_t, lmax, 1);
    if (!*flag) return;
    PAR(tid) { if (tid == 0) lmax[0] = 0; }
    const uint64_t base = (uint64_t)K_BLOCK_IDX * RUN_CHUNK;
    TL_DECL(uint64_t, r, RUN_PER);
    PAR(tid) {
        uint64_t head = RUN_LINKED;                                // first unlinked value among my blocks
        for (uint32_t k = 0; k < RUN_PER; ++k) {
            const uint64_t b = base + (uint64_t)tid * RUN_PER + k;
            TL(r, tid, k) = b < entries ? R[b] : 0;
        }
        for (int k = RUN_PER - 1; k >= 0; --k) if (TL(r, tid, k) != RUN_LINKED) head = TL(r, tid, k);
        v[tid] = head;
    }
    SYNC();
    uint32_t src = 0;
    for (uint32_t d = 1; d < RUN_NT; d <<= 1) {
        PAR(tid) {
            const uint64_t mine = v[src * RUN_NT + tid];
            v[(src ^ 1) * RUN_NT + tid] = (mine == RUN_LINKED && tid + d < RUN_NT) ? v[src * RUN_NT + tid + d] : mine;
        }
        SYNC();
        src ^= 1;
    }
    PAR(tid) {
        uint64_t right = tid + 1 < RUN_NT ? v[src * RUN_NT + tid + 1] : RUN_LINKED;
        if (right == RUN_LINKED) right = carry[K_BLOCK_IDX];
        uint64_t ext = 0;
        for (int k = RUN_PER - 1; k >= 0; --k) {
            const uint64_t b = base + (uint64_t)tid * RUN_PER + k;
            if (TL(r, tid, k) == RUN_LINKED) {
                if (b < entries) R[b] = right;
                const uint64_t e = (right & RUN_POS_MASK) - b * kch;
                ext = e > ext ? e : ext;
            } else right = TL(r, tid, k);
        }
        if (ext >= RUN_LONG) ATOMIC_MAX_LDS_U64(&lmax[0], ext);
    }
    SYNC();
    PAR(tid) { if (tid == 0 && lmax[0]) ATOMIC_MAX_U64(longest, lmax[0]); }
}

// key/sa for an arbitrary list of suffix positions (sample sort, stand-alone entry points).
template <typename idx_t, int BITS>
GLOBAL_FN LAUNCH_BOUNDS(256) make_keys_kernel(KCTX const uint32_t* __restrict__ P, const idx_t* __restrict__ sa, uint64_t cnt,
                                              uint64_t* __restrict__ key)
{
    PAR(tid) {
        const uint64_t i = (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (i < cnt) key[i] = window64<BITS>(P, (uint64_t)sa[i]);
    }
}

// ----------------------------------------------------------------------------------
// Segment descriptors
// ----------------------------------------------------------------------------------

// seg_start[g] = min(g * s, n_total) for g < G, seg_start[G] = n_total
// (subarrays of the reference: src/Suffix_Array.cpp:171-173, the last one takes n % p).
GLOBAL_FN LAUNCH_BOUNDS(256) uniform_segments_kernel(KCTX uint64_t* __restrict__ seg_start, uint32_t G, uint64_t s, uint64_t n_total)
{
    PAR(tid) {
        const uint64_t g = (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (g < G) seg_start[g] = g * s;
        else if (g == G) seg_start[g] = n_total;
    }
}

// seg_start[0 .. 1] = {s0, s1}: ONE segment anywhere in the arrays (a letter-run bucket, pipeline.h sort_run_buckets)
GLOBAL_FN LAUNCH_BOUNDS(64) segment_range_kernel(KCTX uint64_t* __restrict__ seg_start, uint64_t s0, uint64_t s1)
{
    PAR(tid) { if (tid == 0 && K_BLOCK_IDX == 0) { seg_start[0] = s0; seg_start[1] = s1; } }
}

// Exclusive scan of sizes[G] into seg_start[G+1] (single workgroup).
// Partition offsets of the reference's serial scan (src/Suffix_Array.cpp:319-330).
// gfx950: per-wave inclusive scan with wave64 shuffles, wave totals combined through LDS.
GLOBAL_FN LAUNCH_BOUNDS(1024) scan_sizes_kernel(KCTX const uint64_t* __restrict__ sizes, uint32_t G, uint64_t* __restrict__ seg_start)
{
#ifdef CAPS_EMUL
    uint64_t run = 0;
    for (uint32_t g = 0; g < G; ++g) { seg_start[g] = run; run += sizes[g]; }
    seg_start[G] = run;
#else
    __shared__ uint64_t wave_tot[16];
    __shared__ uint64_t carry_s;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t base = 0; base < G; base += 1024) {
        const uint32_t g = base + tid;
        const uint64_t v = g < G ? sizes[g] : 0;
        uint64_t x = v;                                    // inclusive scan inside the wave
        UNROLL
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t y = __shfl_up(x, d, 64);
            if ((int)lane >= d) x += y;
        }
        if (lane == 63) wave_tot[wv] = x;
        __syncthreads();
        uint64_t off = carry_s;
        for (uint32_t w = 0; w < wv; ++w) off += wave_tot[w];
        if (g < G) seg_start[g] = off + x - v;
        __syncthreads();
        if (tid == 1023) carry_s = off + x;
        __syncthreads();
    }
    if (tid == 0) seg_start[G] = carry_s;
#endif
}

// tile_off[G+1] = exclusive scan of ceil(len/TILE_E); out2[0] = #tiles, out2[1] = max segment
// length (out2 must be zeroed before the launch).  Single workgroup; LDS Hillis-Steele scan
// per chunk of 1024 segments.
// skip (optional): segments with skip[g] != 0 get no tiles and do not count for the maximum (they are sorted elsewhere:
// the letter-run buckets of run_bucket_mark_kernel)
GLOBAL_FN LAUNCH_BOUNDS(1024) seg_prepare_kernel(KCTX const uint64_t* __restrict__ seg_start, const uint64_t* __restrict__ seg_end,
                                                 uint32_t G, uint32_t* __restrict__ tile_off, uint64_t* __restrict__ out2,
                                                 const uint8_t* __restrict__ skip)
{
    SHARED_ARRAY(uint32_t, buf, 2048);
    uint32_t carry = 0;
    for (uint32_t base = 0; base < G; base += 1024) {
        PAR(tid) {
            const uint32_t g = base + tid;
            uint64_t len = 0;
            if (g < G && !(skip && skip[g])) len = seg_end_of(seg_start, seg_end, g) - seg_start[g];
            buf[tid] = (uint32_t)((len + TILE_E - 1) / TILE_E);
            if (len) ATOMIC_MAX_U64(&out2[1], len);
        }
        SYNC();
        uint32_t src = 0;
        for (uint32_t d = 1; d < 1024; d <<= 1) {
            PAR(tid) {
                buf[(src ^ 1) * 1024 + tid] = buf[src * 1024 + tid] + (tid >= d ? buf[src * 1024 + tid - d] : 0u);
            }
            SYNC();
            src ^= 1;
        }
        PAR(tid) {
            const uint32_t g = base + tid;
            if (g < G) {
                const uint64_t len = skip && skip[g] ? 0 : seg_end_of(seg_start, seg_end, g) - seg_start[g];
                tile_off[g] = carry + buf[src * 1024 + tid] - (uint32_t)((len + TILE_E - 1) / TILE_E);
            }
        }
        SYNC();
        carry += buf[src * 1024 + 1023];     // block-uniform
        SYNC();
    }
    PAR(tid) {
        if (tid == 0) { tile_off[G] = carry; out2[0] = carry; }
    }
}

// ---- multi-workgroup exclusive scan (segment counts in the millions: the buckets) ------
// block_scan_kernel: workgroup b scans its chunk of SCAN_CHUNK inputs (exclusive, local) and
// records the chunk total; the totals are scanned by scan_sizes_kernel; add_offsets_kernel
// adds them back and writes the grand total to out[n].
constexpr uint32_t SCAN_CHUNK = 4096;

template <typename OutT>
GLOBAL_FN LAUNCH_BOUNDS(1024) block_scan_kernel(KCTX const uint64_t* __restrict__ in, uint64_t n, OutT* __restrict__ out,
                                                uint64_t* __restrict__ sums)
{
    const uint64_t base = (uint64_t)K_BLOCK_IDX * SCAN_CHUNK;
#ifdef CAPS_EMUL
    uint64_t run = 0;
    for (uint32_t i = 0; i < SCAN_CHUNK && base + i < n; ++i) { const uint64_t v = in[base + i]; out[base + i] = (OutT)run; run += v; }
    sums[K_BLOCK_IDX] = run;
#else
    __shared__ uint64_t wave_tot[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint64_t v[4], sum = 0;
    UNROLL
    for (uint32_t i = 0; i < 4; ++i) {
        const uint64_t idx = base + (uint64_t)tid * 4 + i;
        v[i] = idx < n ? in[idx] : 0;
        sum += v[i];
    }
    uint64_t x = sum;
    UNROLL
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t y = __shfl_up(x, d, 64);
        if ((int)lane >= d) x += y;
    }
    if (lane == 63) wave_tot[wv] = x;
    __syncthreads();
    uint64_t run = x - sum;
    for (uint32_t w = 0; w < wv; ++w) run += wave_tot[w];
    UNROLL
    for (uint32_t i = 0; i < 4; ++i) {
        const uint64_t idx = base + (uint64_t)tid * 4 + i;
        if (idx < n) out[idx] = (OutT)run;
        run += v[i];
    }
    if (tid == 1023) sums[blockIdx.x] = run;
#endif
}

template <typename OutT>
GLOBAL_FN LAUNCH_BOUNDS(1024) add_offsets_kernel(KCTX OutT* __restrict__ out, uint64_t n, const uint64_t* __restrict__ offs,
                                                 uint32_t n_chunks)
{
    const uint64_t base = (uint64_t)K_BLOCK_IDX * SCAN_CHUNK;
    const uint64_t off = offs[K_BLOCK_IDX];
    PAR(tid) {
        for (uint32_t i = tid; i < SCAN_CHUNK; i += K_BLOCK_DIM)
            if (base + i < n) out[base + i] = (OutT)((uint64_t)out[base + i] + off);
        if (K_BLOCK_IDX == 0 && tid == 0) out[n] = (OutT)offs[n_chunks];
    }
}

// cnt[g] = ceil(len_g / TILE_E); out2[1] = max len (out2 zeroed before the launch).
GLOBAL_FN LAUNCH_BOUNDS(256) tile_count_kernel(KCTX const uint64_t* __restrict__ seg_start, const uint64_t* __restrict__ seg_end,
                                               uint32_t G, uint64_t* __restrict__ cnt, uint64_t* __restrict__ out2,
                                               const uint8_t* __restrict__ skip)
{
    SHARED_ARRAY(uint64_t, mx, 1);
    PAR(tid) { if (tid == 0) mx[0] = 0; }
    SYNC();
    PAR(tid) {
        const uint64_t g = (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (g < G) {
            const uint64_t len = skip && skip[g] ? 0 : seg_end_of(seg_start, seg_end, g) - seg_start[g];
            cnt[g] = (len + TILE_E - 1) / TILE_E;
            if (len) ATOMIC_MAX_LDS_U64(&mx[0], len);
        }
    }
    SYNC();
    PAR(tid) { if (tid == 0 && mx[0]) ATOMIC_MAX_U64(&out2[1], mx[0]); }
}

// out2[0] = tile_off[G] (number of tiles), for the host read-back.
GLOBAL_FN LAUNCH_BOUNDS(64) tile_total_kernel(KCTX const uint32_t* __restrict__ tile_off, uint32_t G, uint64_t* __restrict__ out2)
{
    PAR(tid) { if (tid == 0 && K_BLOCK_IDX == 0) out2[0] = tile_off[G]; }
}

// tile_rec[b] for the segment g with tile_off[g] <= b < tile_off[g+1].
GLOBAL_FN LAUNCH_BOUNDS(256) tile_map_kernel(KCTX const uint64_t* __restrict__ seg_start, const uint64_t* __restrict__ seg_end,
                                             const uint32_t* __restrict__ tile_off, uint32_t G, TileInfo* __restrict__ tile_rec)
{
    PAR(tid) {
        const uint64_t b = (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (b < tile_off[G]) {
            uint32_t lo = 0, hi = G;               // largest g in [0, G) with tile_off[g] <= b
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) / 2;
                if (tile_off[mid] <= b) lo = mid; else hi = mid;
            }
            TileInfo t;
            t.s0 = seg_start[lo];
            t.s1 = seg_end_of(seg_start, seg_end, lo);
            t.tl = (uint32_t)b - tile_off[lo];
            t.g = lo;
            t.pad_[0] = t.pad_[1] = 0;
            tile_rec[b] = t;
        }
    }
}


// K independent lower-bound searches over LDS-resident sorted (key, sa) runs:
// on return lo[k] = lo[k] + #{elements of [lo[k], hi[k]) that are < (key[k], sa[k])}.
//
// The hot part is branch-free and runs a FIXED number of steps (log2(top), top = a power of
// two > the longest range, block-uniform): step s probes element lo + s - 1 and advances by
// s when it is smaller.  The K probes of a step are independent, so their LDS reads are in
// flight together.  Only keys are compared there (equal key = "not smaller"); a suffix whose
// key also occurs in the range finishes with the exact comparator over the remaining
// candidates -- never on random DNA, routinely on repeats.
template <typename idx_t, int BITS, int K, bool RUNS = true>
DEV_INLINE void multi_lower_bound(const uint32_t* __restrict__ P, uint64_t n, const uint64_t* skey, const idx_t* ssa,
                                  const uint64_t (&key)[K], const idx_t (&sa)[K], uint32_t (&lo)[K], const uint32_t (&hi)[K],
                                  uint32_t top)
{
    for (uint32_t s = top >> 1; s >= 1; s >>= 1) {
        UNROLL
        for (int k = 0; k < K; ++k) {
            const uint32_t idx = lo[k] + s - 1;
            const uint64_t mk = skey[idx < TILE_E ? idx : TILE_E - 1];
            if (idx < hi[k] && mk < key[k]) lo[k] += s;
        }
    }
    UNROLL
    for (int k = 0; k < K; ++k) {
        if (lo[k] < hi[k] && skey[lo[k]] == key[k]) {              // key tie: exact order among [lo, hi)
            uint32_t a = lo[k], b = hi[k];
            while (a < b) {
                const uint32_t mid = (a + b) >> 1;
                if (suffix_less<BITS, RUNS>(P, n, skey[mid], (uint64_t)ssa[mid], key[k], (uint64_t)sa[k])) a = mid + 1;
                else b = mid;
            }
            lo[k] = a;
        }
    }
}

// Deferred ties (pipeline.h SortOpts::defer_ties; msd_* kernels below).  A sort that completes segments of THE suffix array may leave
// the order inside a group of EQUAL keys open: the comparison sort of a tile orders such a group by position (descending: as if
// the text ended behind the key), the merge passes merge by key alone (stably: run A before run B), and the pass that emits the
// LCPs writes TIE_SENTINEL (all ones: no LCP has that value) for every element whose key equals its predecessor's.  The groups
// are then ordered by re-keying them KCH chars deeper, level by level (msd_refine, pipeline.h) -- one window per suffix and level
// instead of a walk through the text per comparison (thousands of suffixes of a tandem array share their first 32 bases and
// agree with their neighbours for ~850 chars: 50 of the 142 ms of the GRCh38-shaped workload were such comparisons).
// K bounds over LDS-resident sorted keys, by key only: lower bound (#{< key}) or upper bound (#{<= key}) per search.
template <int K>
DEV_INLINE void multi_key_bound(const uint64_t* skey, const uint64_t (&key)[K], const bool (&upper)[K], uint32_t (&lo)[K],
                                const uint32_t (&hi)[K], uint32_t top)
{
    for (uint32_t s = top >> 1; s >= 1; s >>= 1) {
        UNROLL
        for (int k = 0; k < K; ++k) {
            const uint32_t idx = lo[k] + s - 1;
            const uint64_t mk = skey[idx < TILE_E ? idx : TILE_E - 1];
            if (idx < hi[k] && (upper[k] ? mk <= key[k] : mk < key[k])) lo[k] += s;
        }
    }
}

// smallest power of two strictly greater than x (x < 2^31)
HD uint32_t pow2_above(uint32_t x) { return 1u << (32 - (x ? __builtin_clz(x) : 32)); }

struct BucketParams {        // per parent segment
    uint64_t kmin;           // smallest key of the segment's range
    uint64_t range;          // largest key - smallest key
    uint32_t shift;          // normalisation: ((key - kmin) << shift) >> 32 spans [0, R32], R32 in [2^31, 2^32)
    uint32_t B;
    uint32_t post;           // bucket = mulhi32(d32, m) >> post, clamped to B - 1
    uint32_t m;
};

// Monotone linear map of [kmin, kmin + range] onto B buckets, in 32-bit arithmetic (the maps run once
// per suffix in four kernels, and a 64 x 64 -> 128 multiply is ~10 quarter-rate VALU instructions):
// d32 = the top 32 bits of the difference, range normalised to [2^31, 2^32); bucket = d32 * B / (R32 + 1).
// The factor B * 2^32 / (R32 + 1) lies in [B, 2B]; it is kept as a 31..32-bit fixed-point number
// (scaled by 2^post), so bucket boundaries are exact to ~2^-31 of the range -- a multiplier with only
// log2(B) significant bits shifts the boundaries by up to 1/B of the range, and the key ranges that
// bucket_ranges_kernel hands to the tile sort no longer match the buckets.
HD BucketParams make_bucket_params(uint64_t kmin, uint64_t kmax, uint32_t B)
{
    BucketParams q;
    q.kmin = kmin;
    q.B = B;
    q.range = kmax > kmin ? kmax - kmin : 0;
    q.shift = q.range ? (uint32_t)caps_clz64(q.range) : 0u;
    const uint64_t r32 = (q.range << q.shift) >> 32;                    // in [2^31, 2^32) unless range == 0
    uint32_t bits = 1;
    while ((2ull * B) >> bits) ++bits;                                  // 2B < 2^bits
    q.post = bits < 32 ? 32 - bits : 0;
    // floor(B * 2^(32 + post) / (r32 + 1)) < 2^32; the numerator is < 2^63 (B < 2^(bits - 1))
    const uint64_t num = (uint64_t)B << (32 + q.post);
    q.m = q.range ? (uint32_t)(num / (r32 + 1)) : 0u;
    return q;
}

DEV_INLINE uint32_t bucket_of(const BucketParams& bp, uint64_t key)
{
    if (bp.B <= 1) return 0;
    if (key <= bp.kmin) return 0;
    const uint64_t d = key - bp.kmin;
    if (d >= bp.range) return bp.B - 1;                               // at or above the top of the nominal range
    const uint32_t d32 = (uint32_t)((d << bp.shift) >> 32);
    const uint32_t b = caps_umul32hi(d32, bp.m) >> bp.post;
    return b < bp.B ? b : bp.B - 1;
}

// ---- slot keys: what level B of the direct path hands to the tile sort in 8-byte records (CAPS_SA_SLOT_KEYS) ----------------
// A bucket of a group with map bp holds the keys of ONE contiguous interval no wider than W = bp.range / bp.B + 1 (the preimage
// of one bucket under the monotone bucket_of), and all of them share their top bits: those need not travel.  The slot holds
//     r = (uint32_t)(key >> s),    s = slot_key_shift(bp.range, bp.B) = max(0, bitlength(W) - 30)         (one shift per group)
// so 2^(30 + s) > W and the window 2^(32 + s) of r is more than four bucket widths.  With l the nominal lower end of the bucket
// (bucket_ranges_kernel: the kmin of its bin map) and
//     base = slot_key_base(l, s) = max(0, l - 2^(30 + s))                                                 (0 when 30 + s >= 64)
// every key k of the bucket satisfies 0 <= (k >> s) - (base >> s) < 2^32, hence x = r - (uint32_t)(base >> s), in 32-bit
// wrap-around arithmetic, is monotone in k whichever multiple of 2^(32 + s) the bucket straddles, and k >> s == (base >> s) + x
// as a 64-bit sum: slot_key_restore gives back k with its low s bits cleared.  Two elements with different x differ in their top
// 64 - s bits (order and LCP as from the 64-bit keys, bit for bit); equal x = the first (64 - s) / BITS chars agree and the text
// decides from there.  The rule is THIS function in both places: the scatter derives s from bps[g], bucket_ranges_kernel stores
// it per bucket in kshift[] for the tile sort.
HD uint32_t slot_key_shift(uint64_t range, uint32_t B)
{
    const uint64_t w = range / (B ? B : 1u);                             // W - 1
    const uint32_t bl = w == ~0ull ? 65u : 64u - (uint32_t)caps_clz64(w + 1);   // bitlength(W)
    return bl > 30u ? bl - 30u : 0u;
}
HD uint64_t slot_key_base(uint64_t l, uint32_t s)
{
    if (30u + s >= 64u) return 0;
    const uint64_t m = 1ull << (30u + s);
    return l > m ? l - m : 0;
}
HD uint64_t slot_key_restore(uint64_t base, uint32_t s, uint32_t r)
{
    const uint64_t bs = base >> s;
    return (bs + (uint32_t)(r - (uint32_t)bs)) << s;
}
// kshift[g] through the scalar unit: the aligned word that holds the byte.  (A byte load from a uniform address is a VECTOR load
// on gfx950, and the wait for it -- the shift is wanted in a scalar register -- would also wait for every data load issued before
// it.)  REQUIRES a table that starts at a multiple of 4 bytes and whose last word can be read: pipeline.h plan() starts every table
// at a multiple of 256 bytes and puts another one behind this one.
DEV_INLINE uint32_t slot_kshift_of(const uint8_t* __restrict__ kshift, uint32_t g)
{
    return (reinterpret_cast<const uint32_t*>(kshift)[g >> 2] >> (8u * (g & 3u))) & 0xFFu;
}
// the record of a slot: r in the low word, the index in the high one (one 8-byte store, one 8-byte load)
HD uint64_t slot_rec(uint64_t key, uint32_t s, uint32_t sa) { return ((uint64_t)sa << 32) | (uint32_t)(key >> s); }

// Exclusive scan of NBINS counters in LDS, in place; h[NBINS] = total.
// gfx950: every thread owns NBINS / TILE_NT consecutive counters; wave64 shuffle scan of the
// per-thread sums, wave totals combined through LDS (two barriers).
template <uint32_t NBINS>
DEV_INLINE void block_exclusive_scan(KCTX uint32_t* h)
{
#ifdef CAPS_EMUL
    (void)kctx_;
    // the same barrier structure as the product code below (the race detector of tests/emul counts on it): every counter is read,
    // barrier, every sum is written, barrier
    std::vector<uint32_t> c(NBINS);
    for (uint32_t i = 0; i < NBINS; ++i) c[i] = h[i];
    SYNC_LDS();
    uint32_t run = 0;
    for (uint32_t i = 0; i < NBINS; ++i) { h[i] = run; run += c[i]; }
    h[NBINS] = run;
    SYNC_LDS();
#else
    constexpr uint32_t BPT = NBINS / TILE_NT;
    static_assert(BPT >= 1 && BPT * TILE_NT == NBINS, "counters per thread");
    __shared__ uint32_t wave_tot[TILE_NT / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint32_t v[BPT], sum = 0;
    UNROLL
    for (uint32_t i = 0; i < BPT; ++i) { v[i] = h[tid * BPT + i]; sum += v[i]; }
    // inclusive scan over the wave with DPP moves (rows of 16 lanes: shifts by 1, 2, 4, 8; then the last lane of row 0 / 2 into
    // row 1 / 3, and lane 31 into rows 2 and 3): six move + add pairs.  (__shfl_up costs an index computation and a
    // ds_bpermute per step: the four scans of a tile were ~10 % of tile_sort_eq_kernel's instructions.)
    uint32_t x = sum;
#define CAPS_DPP_ADD(ctrl, rows) x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, ctrl, rows, 0xF, false)
    CAPS_DPP_ADD(0x111, 0xF);        // row_shr:1
    CAPS_DPP_ADD(0x112, 0xF);        // row_shr:2
    CAPS_DPP_ADD(0x114, 0xF);        // row_shr:4
    CAPS_DPP_ADD(0x118, 0xF);        // row_shr:8
    CAPS_DPP_ADD(0x142, 0xA);        // row_bcast:15 -> rows 1 and 3
    CAPS_DPP_ADD(0x143, 0xC);        // row_bcast:31 -> rows 2 and 3
#undef CAPS_DPP_ADD
    if (lane == 63) wave_tot[wv] = x;
    SYNC_LDS();
    uint32_t run = x - sum;
    if (TILE_NT / 64 <= 16) {
        // the waves' totals: lanes 0 .. 15 hold one each, prefix by DPP within the row, this wave's through readlane
        const uint32_t wt = lane < TILE_NT / 64 ? wave_tot[lane] : 0u;
        uint32_t ws = wt;
#define CAPS_DPP_ADD(ctrl) ws += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)ws, ctrl, 0xF, 0xF, false)
        CAPS_DPP_ADD(0x111);
        CAPS_DPP_ADD(0x112);
        CAPS_DPP_ADD(0x114);
        CAPS_DPP_ADD(0x118);
#undef CAPS_DPP_ADD
        const int wvs = __builtin_amdgcn_readfirstlane((int)wv);
        run += (uint32_t)__builtin_amdgcn_readlane((int)ws, wvs) - (uint32_t)__builtin_amdgcn_readlane((int)wt, wvs);
    } else {
        for (uint32_t w = 0; w < wv; ++w) run += wave_tot[w];
    }
    UNROLL
    for (uint32_t i = 0; i < BPT; ++i) { h[tid * BPT + i] = run; run += v[i]; }
    if (tid == TILE_NT - 1) h[NBINS] = run;
    SYNC_LDS();
#endif
}
DEV_INLINE void block_exclusive_scan_bins(KCTX uint32_t* hist) { block_exclusive_scan<TILE_BINS_>(KCTX_PASS hist); }

// Final destination of a sort whose result is THE suffix / LCP array (phase 2): SA and LCP slots
// of the caller plus, per sorted segment, its first and last (key, sa) -- the boundary records
// from which head_lcp_kernel computes the LCP at every segment head (a11).
template <typename idx_t> struct FinalOut {
    idx_t* sa = nullptr;
    idx_t* lcp = nullptr;
    uint64_t* first_key = nullptr;
    uint64_t* last_key = nullptr;
    idx_t* first_sa = nullptr;
    idx_t* last_sa = nullptr;
};

// Bins of the in-LDS bucket sort of one tile, and the bin occupancy above which the tile
// falls back to the merge levels.
#ifdef CAPS_EMUL
extern "C" void caps_emul_count_tile(bool fast, bool known_range);   // test statistics (tests/emul/emul_lib.cpp)
extern "C" void caps_emul_count_tile2(bool two_level_ok);
extern "C" void caps_emul_count_tile3(bool equalised_ok);
#endif
constexpr uint32_t TILE_BINS = TILE_BINS_;
// Largest bin the exact in-bin ranking (quadratic in the bin) accepts: in tile_sort_kernel, whose linear map either
// works (uniform keys: bins of 2-3) or is hopeless, and in tile_sort_eq_kernel, the last stop before the comparison sort.
#ifndef CAPS_TILE_BIN_LIMIT
#define CAPS_TILE_BIN_LIMIT 48    /* genome-like 3e9: 16 / 24 / 48 / 128 -> 300 / 301 / 299 / 320 ms (the eq kernel sorts crowded tiles cheaper than a quadratic ranking of big bins) */
#endif
#ifndef CAPS_EQ_BIN_LIMIT
#define CAPS_EQ_BIN_LIMIT 128
#endif
constexpr uint32_t TILE_BIN_LIMIT = CAPS_TILE_BIN_LIMIT;
constexpr uint32_t EQ_BIN_LIMIT = CAPS_EQ_BIN_LIMIT;

// ----------------------------------------------------------------------------------
// a4/a5: tile sort -- one workgroup sorts up to TILE_E suffixes in LDS and emits the
// sorted run with its LCP array (reference: merge_sort, src/Suffix_Array.cpp:112-129,
// called per subarray at :171-173).
//
// FROM_TEXT: the tile is TILE_E consecutive text positions (phase 1), element i of the
// arrays being text position text_base + i (text_base != 0 on a shard that owns a slice of
// the subarrays); keys are cut from the packed text.  Otherwise (key, sa) pairs are read
// from in_key/in_sa.
// In-LDS algorithm: bottom-up merge sort where every element finds its output slot
// by a binary search in the sibling run (rank merge): no divergent serial merge,
// ragged runs need no padding.  LCPs are produced once, at the end, from adjacent
// keys (text only on equal keys).
// LDS: TILE_E x (8 + sizeof(idx_t)).
// ----------------------------------------------------------------------------------
// LCP of two neighbours of a sorted tile from their keys, 64-bit or 32-bit (text.h); cs: the 32-bit keys' shift
// min(l, chars the shorter of the suffixes a, b has), in the width of the indices: with 32-bit indices n < 2^32, and the
// 64-bit max / subtract / min of the generic form are a tenth of tile_sort_kernel's instructions per suffix
template <typename idx_t>
DEV_INLINE uint64_t lcp_capped(uint32_t l, uint64_t n, idx_t a, idx_t b)
{
    if (sizeof(idx_t) == 4) {
        const uint32_t room = (uint32_t)n - (uint32_t)(a > b ? a : b);
        return l < room ? l : room;
    }
    const uint64_t room = n - (uint64_t)(a > b ? a : b);
    return l < room ? l : room;
}
template <int BITS, bool RUNS, typename idx_t>
DEV_INLINE uint64_t tile_pair_lcp(const uint32_t* __restrict__ P, uint64_t n, uint64_t ka, idx_t a, uint64_t kb, idx_t b, uint32_t)
{
    const uint64_t x = ka ^ kb;
    if (x) return lcp_capped<idx_t>((uint32_t)caps_clz64(x) / BITS, n, a, b);
    return pair_lcp<BITS, RUNS>(P, n, ka, (uint64_t)a, kb, (uint64_t)b);
}
template <int BITS, bool RUNS, typename idx_t>
DEV_INLINE uint64_t tile_pair_lcp(const uint32_t* __restrict__ P, uint64_t n, uint32_t ka, idx_t a, uint32_t kb, idx_t b, uint32_t cs)
{
    return pair_lcp32<BITS, RUNS>(P, n, ka, (uint64_t)a, kb, (uint64_t)b, cs);
}

// ... of two keys put together from slot keys (tile_sort_kernel SLOTREC): equal keys stand for `from` equal chars, not KCH
template <int BITS, typename idx_t>
DEV_INLINE uint64_t slot_pair_lcp(const uint32_t* __restrict__ P, uint64_t n, uint64_t ka, idx_t a, uint64_t kb, idx_t b, uint32_t from)
{
    const uint64_t x = ka ^ kb;
    if (x) return lcp_capped<idx_t>((uint32_t)caps_clz64(x) / BITS, n, a, b);
    return deep_lcp<BITS, false>(P, n, (uint64_t)a, (uint64_t)b, from);
}

// ... or TIE_SENTINEL for a pair of equal keys when ties are deferred (bflag != null: "Deferred ties" above)
template <typename idx_t> HD idx_t tie_sentinel() { return (idx_t)~(idx_t)0; }
template <int BITS, bool RUNS, typename idx_t>
DEV_INLINE uint64_t deferring_pair_lcp(const uint32_t* __restrict__ P, uint64_t n, uint64_t* __restrict__ bflag, uint32_t g, uint64_t ka, idx_t a,
                                       uint64_t kb, idx_t b)
{
    if (bflag && ka == kb) { bflag[g] = 1; return (uint64_t)tie_sentinel<idx_t>(); }       // (benign race: every writer stores 1)
    return tile_pair_lcp<BITS, RUNS>(P, n, ka, a, kb, b, 0u);
}

// Measurement only (make variant VARIANT_DEFS=-DCAPS_PHASE_CLOCK; never in the product build): thread 0 of every workgroup
// adds the cycles between two marks to caps_phase_clock[slot] -- which barrier-separated phase of a tile sort takes the time
// (tools/phase_clock.py reads the counters through caps_sa_hip_phase_clock()).  The results of the kernels are unchanged.
#if defined(CAPS_PHASE_CLOCK) && !defined(CAPS_EMUL)
__device__ unsigned long long caps_phase_clock[32];
#define PHASE_T0() unsigned long long pc_t_ = clock64()
#define PHASE_MARK(i) do { const unsigned long long t_ = clock64(); if (threadIdx.x == 0) atomicAdd(&caps_phase_clock[i], t_ - pc_t_); pc_t_ = clock64(); } while (0)
#else
#define PHASE_T0() ((void)0)
#define PHASE_MARK(i) ((void)0)
#endif

// Debugging only (make variant VARIANT_DEFS=-DCAPS_EQ_CHECK): every index tile_sort_eq_kernel derives from data it was handed (queue
// entries, tile records, slots, bins, suffix positions) is range-checked; a failed check is counted in caps_eq_check[id] (read
// out through caps_sa_hip_eq_check()) and the access is skipped or clamped instead of made -- so a wild index shows up as a
// number rather than as a memory access fault.  Never in the product build.
#if defined(CAPS_EQ_CHECK) && !defined(CAPS_EMUL)
__device__ unsigned int caps_eq_check[64];
#define EQ_OK(ok, id) ((ok) ? true : (atomicAdd(&caps_eq_check[id], 1u), false))
#else
#define EQ_OK(ok, id) (true)
#endif
#define EQ_CHK(ok, id) ((void)EQ_OK((ok), (id)))

// (key, index) as ONE element: what level A of the direct path hands to level B at 32-bit indices.  A run that a tile appends to
// a stream is then one contiguous segment of 12-byte records instead of a segment of keys and, elsewhere, a segment of
// indices: fewer cache lines touched per run, one store and one load per element instead of two.  4-byte aligned (a stream
// starts anywhere); a copy compiles to one 12-byte load and one 12-byte store.  The region of a stream holds the same number of
// elements and bytes as in the two-array layout.
struct __attribute__((packed, aligned(4))) KeySaRec {
    uint32_t key_lo, key_hi;
    uint32_t sa;
};
static_assert(sizeof(KeySaRec) == 12 && alignof(KeySaRec) == 4, "12-byte records");
#ifdef CAPS_EMUL
DEV_INLINE KeySaRec rec_stream_load(const KeySaRec* p) { return *p; }
#elif !defined(CAPS_NO_STREAM_HINTS)
typedef uint32_t caps_u32x3 __attribute__((ext_vector_type(3)));
typedef caps_u32x3 caps_u32x3_a4 __attribute__((aligned(4)));
DEV_INLINE KeySaRec rec_stream_load(const KeySaRec* p)       // read once: nontemporal, as STREAM_LOAD
{
    const caps_u32x3 v = __builtin_nontemporal_load(reinterpret_cast<const caps_u32x3_a4*>(p));
    KeySaRec r;
    r.key_lo = v.x; r.key_hi = v.y; r.sa = v.z;
    return r;
}
#else
DEV_INLINE KeySaRec rec_stream_load(const KeySaRec* p) { return *p; }
#endif
template <typename KP, typename idx_t> DEV_INLINE void store_rec(KP* out, uint64_t i, uint64_t key, idx_t sa)
{
    // one plain 12-byte store (never nontemporal: the short runs of level A complete each other's lines in L2)
    KeySaRec r;
    r.key_lo = (uint32_t)key; r.key_hi = (uint32_t)(key >> 32); r.sa = (uint32_t)sa;
    reinterpret_cast<KeySaRec*>(out)[i] = r;
}

// Where a tile of a sort over slots reads its keys: the slot array, or -- a bucket that outgrew its slot (speculative split by
// knots: spill_gather_kernel / spill_place_kernel have put it together there) -- its place in the output array, sorted in place.
// (32-bit keys live in slots only: such a sort gives up when a slot overflows.)
DEV_INLINE const uint64_t* tile_src(const uint64_t* in, const uint64_t* out, bool from_out) { return from_out ? out : in; }
DEV_INLINE const uint32_t* tile_src(const uint32_t* in, const uint64_t*, bool) { return in; }

// Shared pieces of the two tile sort kernels (macros: they use the kernels' TL registers).
// (The start of a tile -- which segment, where its input sits, whether it emits LCPs -- is written out in tile_sort_kernel,
// "the start of a tile" there; the other tile kernels derive the same values for the tile they took from their queue.)
#define TILE_OUTGROWN (slot_cap != 0 && t.s1 - t.s0 > (uint64_t)slot_cap)

#define TILE_SRC_KEY in_key
#define TILE_SRC_SA in_sa
/* (tile_sort_kernel's bucket-indexed build has a copy of the clears of flag and hist below -- without kmm, which it never reads --    */
/* next to its late load: a word added to the clears here is added there.)                                                       */
#define TILE_SORT_LOAD                                                                                          \
    PAR(tid) {                                                                                                  \
        if (tid == 0) { kmm[0] = ~0ull; kmm[1] = 0; flag[0] = 0; }                                              \
        for (uint32_t i = tid; i <= TILE_BINS; i += K_BLOCK_DIM) hist[i] = 0;                                   \
        UNROLL                                                                                                  \
        for (uint32_t k = 0; k < TILE_EPT; ++k) {                                                               \
            const uint32_t e = tid + k * TILE_NT;                                                               \
            if (e < cnt) {                                                                                      \
                uint64_t key;                                                                                   \
                idx_t sa;                                                                                       \
                if (FROM_TEXT) {                                                                                \
                    key = window64<BITS>(P, text_base + start + e);                                             \
                    sa = (idx_t)(text_base + start + e);                                                        \
                } else if (TILE_KEYS_FROM_TEXT) {   /* 32-bit keys in the slots: the 64-bit key is cut from the text */ \
                    sa = STREAM_LOAD(&TILE_SRC_SA[in0 + e]);                                                    \
                    key = window64<BITS>(P, (uint64_t)sa);                                                      \
                } else {                                                                                        \
                    key = STREAM_LOAD(&TILE_SRC_KEY[in0 + e]);                                                  \
                    sa = STREAM_LOAD(&TILE_SRC_SA[in0 + e]);                                                    \
                }                                                                                               \
                TL(rk, tid, k) = (decltype(TL(rk, tid, k) + 0))key;                                             \
                TL(rs, tid, k) = sa;                                                                            \
            }                                                                                                   \
        }                                                                                                       \
    }

// Bin map of the tile: prepared in advance when the tile belongs to a key-range bucket (seg_map, from
// bucket_ranges_kernel: its 64-bit division would otherwise be repeated by every thread of every
// tile), otherwise from the min / max over the tile.
/* TILE_SYNC: the barrier of the tile kernels' shared pieces.  Everything the threads of a tile hand each other goes through  */
/* LDS, so tile_sort_eq_kernel (which keeps spilled registers in scratch and emits straight before its next tile) uses the  */
/* LDS-scope barrier: __syncthreads() would also wait for every scratch store and every result store of the wave.           */
#define TILE_SYNC() SYNC()
#define TILE_SORT_RANGE TILE_SORT_RANGE_(seg_map[g])
/* MAP: the prepared bin map of segment g (tile_sort_kernel's bucket-indexed build has loaded it ahead of the barrier) */
#define TILE_SORT_RANGE_(MAP)                                                                                   \
    const bool known_range = seg_map != nullptr;                                                                \
    if (!known_range) {                                                                                         \
        TILE_SYNC(); /* kmm initialised */                                                                      \
        PAR(tid) {                                                                                              \
            uint64_t mn = ~0ull, mx = 0;                                                                        \
            UNROLL                                                                                              \
            for (uint32_t k = 0; k < TILE_EPT; ++k) {                                                           \
                const uint32_t e = tid + k * TILE_NT;                                                           \
                if (e < cnt) {                                                                                  \
                    const uint64_t key = (uint64_t)TL(rk, tid, k);                                              \
                    mn = key < mn ? key : mn;                                                                   \
                    mx = key > mx ? key : mx;                                                                   \
                }                                                                                               \
            }                                                                                                   \
            BLOCK_MINMAX_U64(&kmm[0], &kmm[1], mn, mx);                                                         \
        }                                                                                                       \
    }                                                                                                           \
    TILE_SYNC();                                                                                                \
    const BucketParams tb = known_range ? (MAP) : make_bucket_params(kmm[0], kmm[1], TILE_BINS); /* block-uniform */

// registers -> final slots TL(rd) in LDS
#define TILE_SORT_PLACE_FINAL                                                                                   \
    PAR(tid) {                                                                                                  \
        UNROLL                                                                                                  \
        for (uint32_t k = 0; k < TILE_EPT; ++k) {                                                               \
            const uint32_t e = tid + k * TILE_NT;                                                               \
            if (e < cnt) {                                                                                      \
                const uint32_t d = TL(rd, tid, k);                                                              \
                skey[d] = TL(rk, tid, k);                                                                       \
                ssa[d] = TL(rs, tid, k);                                                                        \
            }                                                                                                   \
        }                                                                                                       \
    }                                                                                                           \
    TILE_SYNC();

// sorted tile in LDS -> HBM (+ LCPs from adjacent keys, + boundary records)
#define TILE_SORT_EMIT TILE_SORT_EMIT_(0u)
/* OV: an lcp already known for slot e (0 = none: from the keys, the text on equal keys) */
#define TILE_EMIT_LCP_(ka, a, kb, b) tile_pair_lcp<BITS, TILE_RUNS>(P, n, ka, a, kb, b, TILE_KEY_SHIFT)
#define TILE_SORT_EMIT_(OV)                                                                                     \
    PAR(tid) {                                                                                                  \
        UNROLL                                                                                                  \
        for (uint32_t k = 0; k < TILE_EPT; ++k) {                                                               \
            const uint32_t e = tid + k * TILE_NT;                                                               \
            if (e < cnt) {                                                                                      \
                const uint64_t key = skey[e];                                                                   \
                const idx_t sa = ssa[e];                                                                        \
                uint64_t l = 0;                                                                                 \
                if (with_lcp && e) {                                                                            \
                    const uint32_t ov_ = (OV);                                                                  \
                    l = ov_ ? ov_ : TILE_EMIT_LCP_(skey[e - 1], ssa[e - 1], skey[e], sa);                          \
                }                                                                                               \
                if (direct) {                                                                                   \
                    STREAM_STORE(&fin.sa[start + e], sa);                                                       \
                    STREAM_STORE(&fin.lcp[start + e], (idx_t)l);                                                \
                    if (e == 0) { fin.first_key[g] = key; fin.first_sa[g] = sa; }                               \
                    if (e == cnt - 1) { fin.last_key[g] = key; fin.last_sa[g] = sa; }                           \
                } else {                                                                                        \
                    out_key[start + e] = key;                                                                   \
                    out_sa[start + e] = sa;                                                                     \
                    if (with_lcp) out_lcp[start + e] = (idx_t)l;                                                \
                }                                                                                               \
            }                                                                                                   \
        }                                                                                                       \
    }

// ---- tile_sort_kernel: interpolation bucket sort in LDS ------------------------------
// bin = monotone linear map of the key onto TILE_BINS bins over the tile's key range; a
// counting sort by bin (LDS histogram + scan) places every element next to the few others of
// its bin, and a short exact scan of its own bin fixes the order.  ~100 VALU instructions per
// suffix instead of ~1000 for a comparison sort.  Completes the tile when no bin holds more than
// TILE_BIN_LIMIT elements (always on keys that are roughly uniform in their range: random DNA,
// buckets of the bucketing stage); otherwise it writes nothing and sets redo[tile], and
// tile_sort_general_kernel sorts the tile.
// KT = uint32_t: the slots hold 32-bit keys (text.h key32_of; kshift[bucket] = the shift of the bucket's group).  Only
// completed segments written straight to SA / LCP (`direct`) exist then; a tile this kernel cannot finish is re-sorted by the
// kernels below from 64-bit keys cut from the text.
// CHAIN != 0: the bucket-indexed build, for a sort over slots of TILE_E elements in which every bucket fits its slot (a bucket is
// then exactly one tile, its input sits at g * slot_cap whatever the tables say): workgroup g takes bucket g, and its first
// instructions are the loads of the slot -- a tile of the table launch starts with two dependent round trips before them (its tile
// record, then the slot the record names).  The bucket's bounds and its bin map are fetched while those loads are in flight; an
// empty bucket returns; lanes at or beyond the bucket's size keep whatever the (allocated) slot held, every later phase is guarded
// by e < cnt.  All but the last of the TILE_EPT loads per thread are issued ahead of the bounds, the last once cnt is known: a
// bucket fills 7/8 of its slot, and loading the whole slot early -- 5 GB more at 3e9 -- took back most of the gain.
// The queue of unfinished tiles still carries tile indices (the kernels behind this one read their tiles through tile_rec):
// tile_off[g].  grid = the slots.
// SLOTREC (CHAIN != 0): the slots hold 8-byte records of slot keys ("slot keys" above; in_key points at them, in_sa is unused,
// kshift[bucket] = the shift of the bucket's group).  Only the load differs: one 8-byte load per element, and behind the wait
// the 64-bit key is put together again from the record, the shift and the bucket's nominal lower end (the kmin of its bin map)
// -- with its low `shift` bits cleared.  From there this is the 64-bit kernel, except that equal keys stand for tie_from =
// (64 - shift) / BITS equal chars instead of KCH: the tie-break and the LCP of such a pair read the text from there.  A tile
// this build cannot finish is queued as ever; the kernels behind it cut their keys from the text (slot_unpack_kernel).
template <typename idx_t, int BITS, bool FROM_TEXT, typename KT = uint64_t, int CHAIN = 0, bool SLOTREC = false>
GLOBAL_FN LAUNCH_BOUNDS2(TILE_NT, TILE_WAVES_PER_SIMD) tile_sort_kernel(KCTX SegDesc sd, const uint32_t* __restrict__ P, uint64_t n,
                                                  uint64_t text_base, uint32_t lcp_mode, uint32_t slot_cap, const KT* in_key,
                                                  const idx_t* in_sa, uint64_t* out_key, idx_t* out_sa, idx_t* out_lcp,
                                                  FinalOut<idx_t> fin, const BucketParams* __restrict__ seg_map,
                                                  uint32_t* __restrict__ redo, const uint8_t* __restrict__ kshift)
{
    constexpr bool TILE_RUNS = false;        // ties here are shallow (suffix_less_tie_bounded), so are the LCPs
    constexpr bool K32 = sizeof(KT) == 4;
    constexpr bool TILE_KEYS_FROM_TEXT = false;
    constexpr bool BY_BUCKET = CHAIN != 0;
    constexpr uint32_t CHAIN_EARLY = BY_BUCKET ? TILE_EPT - 1 : 0u;
    static_assert(!K32 || !FROM_TEXT, "32-bit keys come from the slots of level B");
    static_assert(!BY_BUCKET || (!FROM_TEXT && !K32 && sizeof(idx_t) == 4), "bucket-indexed: 64-bit keys and 32-bit indices in slots");
    static_assert(!SLOTREC || (BY_BUCKET && BITS == 2), "records of slot keys: the bucket-indexed build on 2-bit texts");
    TL_DECL(KT, rk, TILE_EPT);
    TL_DECL(idx_t, rs, TILE_EPT);
    uint64_t bs0 = 0, bs1 = 0;                                              // BY_BUCKET: the bucket's bounds and its bin map, requested
    BucketParams tb_early = BucketParams();                                 //   here and not waited for before the loads below are out
    uint32_t ks_early = 0;                                                  // SLOTREC: ... and the shift of the bucket's slot keys
    // BY_BUCKET REQUIRES seg_map (one prepared bin map per slot of the grid) and seg_start[0 .. grid]: the launch reads both
    // unconditionally, and this build does not initialise kmm -- the min / max route of TILE_SORT_RANGE_ (seg_map == null) would
    // read it unset.  segmented_sort takes this launch only with seg_map != null and grid <= G (pipeline.h, by_bucket).
    if (BY_BUCKET) {
        bs0 = sd.seg_start[K_BLOCK_IDX];
        bs1 = sd.seg_start[K_BLOCK_IDX + 1];
        tb_early = seg_map[K_BLOCK_IDX];
        if (SLOTREC) ks_early = slot_kshift_of(kshift, K_BLOCK_IDX);
        PAR(tid) {
            const uint64_t in0e = (uint64_t)K_BLOCK_IDX * slot_cap;
            UNROLL
            for (uint32_t k = 0; k < CHAIN_EARLY; ++k) {
                TL(rk, tid, k) = STREAM_LOAD(&in_key[in0e + tid + k * TILE_NT]);                  // (SLOTREC: the record)
                if (!SLOTREC) TL(rs, tid, k) = STREAM_LOAD(&in_sa[in0e + tid + k * TILE_NT]);
            }
        }
        ISSUE_FENCE();                                                        // ... and stay ahead of the branch on the bounds
    }
    // ---- the start of a tile ----
    const uint32_t b = K_BLOCK_IDX;                                           // the tile, or (BY_BUCKET) the bucket
    if (!BY_BUCKET && b >= sd.tile_off[sd.G]) return;
    const uint32_t g = BY_BUCKET ? b : sd.tile_rec[b].g;
    const TileInfo t = BY_BUCKET ? TileInfo{bs0, bs1, 0u, g, {0u, 0u}} : tile_info(sd, b);
    if (BY_BUCKET && t.s1 == t.s0) return;
    const uint64_t start = t.s0 + (uint64_t)t.tl * TILE_E;
    const uint32_t cnt = (uint32_t)(t.s1 - start < TILE_E ? t.s1 - start : TILE_E);
    // LCPs are only needed from the sort that completes a segment: lcp_mode 0 = never, 1 = when the whole segment is this tile
    // (otherwise its final merge pass emits them).
    const bool with_lcp = lcp_mode != 0 && (t.s1 - t.s0) <= TILE_E;
    // fin.sa != null: a segment completed here goes straight to the caller's SA / LCP arrays (its head LCP is filled in by
    // head_lcp_kernel from the boundary records).
    const bool direct = with_lcp && fin.sa != nullptr;
    // slot_cap != 0: the input of segment (bucket) g sits in its fixed-capacity slot, see bucket_scatter_kernel.  (A bucket that
    // outgrew its slot -- speculative split by knots -- was put together at its place in the OUTPUT arrays: TILE_OUTGROWN.  The
    // kernels at the head of the queue chain never see such a tile: the tile table they are launched with shows it EMPTY
    // (hot_tiles_kernel), they pass it on as unfinished, and the builds behind them -- launched with the true table -- read it
    // there, tile_src above.  No code for it here: a test in tile_sort_eq_kernel's plain build cost ten more SGPR spills and 5 %
    // of its time.)
    const uint64_t in0 = slot_cap ? (uint64_t)g * slot_cap : start;
    const uint32_t TILE_KEY_SHIFT = K32 ? kshift[g] : 0u;                                  // block-uniform
    const uint32_t tie_from = K32       ? (TILE_KEY_SHIFT + 32u) / BITS                    // chars two equal keys stand for
                              : SLOTREC ? (64u - ks_early) / BITS
                                        : TextTraits<BITS>::KCH;
    SHARED_ARRAY(KT, skey, TILE_E);
    SHARED_ARRAY(idx_t, ssa, TILE_E);
    SHARED_ARRAY(uint32_t, hist, TILE_BINS + 1);
    SHARED_ARRAY(uint64_t, kmm, 2);          // min / max key of the tile
    SHARED_ARRAY(uint32_t, flag, 1);         // a bin overflowed
    // SLOT_ORDER: from the rank phase on a thread works on the elements in slots tid + k * TILE_NT instead of the ones it
    // loaded (their bins: sbin).  The lanes of a wave then hold neighbouring slots -- mostly one bin or two: the keys they scan
    // are the same LDS words (one read serves all), the loops have the same length, and the final placement moves every
    // element a few slots, neighbours to neighbours, where the loaded elements sat in 64 bins all over the tile (half of
    // this kernel's LDS cycles were bank conflicts).  64-bit indices: no room in LDS (two workgroups per CU) for sbin.
    constexpr bool SLOT_ORDER = sizeof(idx_t) == 4;
    SHARED_ARRAY(uint16_t, sbin, SLOT_ORDER ? TILE_E : 1);
    // ... and no second placement (as in tile_sort_eq_kernel): the element that knows its final position d notes perm[d] = its slot,
    // the emit phase reads keys and indices through perm -- one barrier, two LDS writes and a read per element less
    SHARED_ARRAY(uint16_t, perm, SLOT_ORDER ? TILE_E : 1);
    TL_DECL(uint32_t, rd, TILE_EPT);
    TL_DECL(uint32_t, rb, TILE_EPT);

    PHASE_T0();
    if (BY_BUCKET) {
        PAR(tid) {
            if (tid == 0) flag[0] = 0;
            for (uint32_t i = tid; i <= TILE_BINS; i += K_BLOCK_DIM) hist[i] = 0;
            UNROLL
            for (uint32_t k = CHAIN_EARLY; k < TILE_EPT; ++k) {
                const uint32_t e = tid + k * TILE_NT;
                if (e < cnt) {
                    TL(rk, tid, k) = STREAM_LOAD(&in_key[in0 + e]);
                    if (!SLOTREC) TL(rs, tid, k) = STREAM_LOAD(&in_sa[in0 + e]);
                }
            }
        }
    } else {
        TILE_SORT_LOAD
    }
    TILE_SORT_RANGE_(BY_BUCKET ? tb_early : seg_map[g])
    if (SLOTREC) {
        // record -> (64-bit key with its low bits cleared, index); lanes at or beyond cnt hold whatever the slot held, as before
        const uint64_t kbase = slot_key_base(tb.kmin, ks_early);
        PAR(tid) {
            UNROLL
            for (uint32_t k = 0; k < TILE_EPT; ++k) {
                if (k >= CHAIN_EARLY && tid + k * TILE_NT >= cnt) continue;                     // (the late load was not made)
                const uint64_t rec = (uint64_t)TL(rk, tid, k);
                TL(rs, tid, k) = (idx_t)(rec >> 32);
                TL(rk, tid, k) = (KT)slot_key_restore(kbase, ks_early, (uint32_t)rec);
            }
        }
    }
    PHASE_MARK(0);                                             // load (+ range)
    bool fast = cnt > 1 && tb.range > 0;
    if (fast) {
        PAR(tid) {
            UNROLL
            for (uint32_t k = 0; k < TILE_EPT; ++k) {
                const uint32_t e = tid + k * TILE_NT;
                if (e < cnt) {
                    const uint32_t bin = bucket_of(tb, TL(rk, tid, k));
                    const uint32_t r = FETCH_ADD_U32(&hist[bin], 1u);
                    if (r >= TILE_BIN_LIMIT) flag[0] = 1;
                    TL(rb, tid, k) = bin;
                    TL(rd, tid, k) = r;
                }
            }
        }
        SYNC();
        fast = flag[0] == 0;
        PHASE_MARK(1);                                         // histogram
    }
    if (cnt == 1) {                              // nothing to sort
        PAR(tid) { if (tid == 0) { skey[0] = TL(rk, tid, 0); ssa[0] = TL(rs, tid, 0); } }
        SYNC();
        fast = true;
    } else if (fast) {
        block_exclusive_scan_bins(KCTX_PASS hist);         // hist[b] = first slot of bin b, hist[TILE_BINS] = cnt
        PHASE_MARK(2);                                         // scan
        PAR(tid) {
            UNROLL
            for (uint32_t k = 0; k < TILE_EPT; ++k) {
                const uint32_t e = tid + k * TILE_NT;
                if (e < cnt) {
                    const uint32_t slot = hist[TL(rb, tid, k)] + TL(rd, tid, k);
                    skey[slot] = TL(rk, tid, k);
                    ssa[slot] = TL(rs, tid, k);
                    if (SLOT_ORDER) sbin[slot] = (uint16_t)TL(rb, tid, k);
                    else TL(rd, tid, k) = slot;
                }
            }
        }
        SYNC();
        PHASE_MARK(3);                                         // place by bin
        PAR(tid) {
            UNROLL
            for (uint32_t k = 0; k < TILE_EPT; ++k) {
                const uint32_t e = tid + k * TILE_NT;
                if (e < cnt) {
                    const uint32_t slot = SLOT_ORDER ? e : TL(rd, tid, k), bin = SLOT_ORDER ? (uint32_t)sbin[slot] : TL(rb, tid, k);
                    const uint32_t bs = hist[bin], be = hist[bin + 1];
                    const uint64_t key = SLOT_ORDER ? (uint64_t)skey[slot] : (uint64_t)TL(rk, tid, k);
                    uint32_t less = 0;                        // members of my bin that sort before me
                    for (uint32_t j = bs; j < be; ++j) {
                        const uint64_t kj = skey[j];
                        less += kj < key ? 1u : 0u;
                        if (kj == key && j != slot) {                                                               // rare: text
                            const uint64_t sa = SLOT_ORDER ? (uint64_t)ssa[slot] : (uint64_t)TL(rs, tid, k);
                            const uint32_t c = suffix_less_tie_bounded<BITS>(P, n, (uint64_t)ssa[j], sa, tie_from);
                            if (c == 2u) flag[0] = 1;                                                               // a deep tie: not here
                            less += c & 1u;
                        }
                    }
                    // (bs + less < be <= cnt whatever the ties did; RACY_STORE: two members of a tie too deep for this kernel get one
                    // rank and one cell -- the tile has raised its flag by then and nothing reads perm)
                    if (SLOT_ORDER) RACY_STORE_U16(&perm[bs + less], (uint16_t)slot);
                    else TL(rd, tid, k) = bs + less;
                }
            }
        }
        SYNC();
        fast = flag[0] == 0;
        PHASE_MARK(4);                                         // rank inside the bin
        if (fast && !SLOT_ORDER) {
            TILE_SORT_PLACE_FINAL
            PHASE_MARK(5);                                     // place final
        }
    }
#ifdef CAPS_EMUL
    caps_emul_count_tile(fast, known_range);
#endif
    // unfinished: queue the tile for tile_sort_general_kernel (redo[0] = queue length)
    if (!fast) {
        PAR(tid) { if (tid == 0) redo[1 + FETCH_ADD_U32(&redo[0], 1u)] = BY_BUCKET ? sd.tile_off[g] : b; }
        return;
    }
    if (SLOT_ORDER && cnt > 1) {
        // sorted order -> HBM through perm (+ LCPs from neighbouring keys, + boundary records)
        PAR(tid) {
            UNROLL
            for (uint32_t k = 0; k < TILE_EPT; ++k) {
                const uint32_t e = tid + k * TILE_NT;
                if (e < cnt) {
                    const uint32_t sl = perm[e];
                    const KT key = skey[sl];
                    const idx_t sa = ssa[sl];
                    uint64_t l = 0;
                    if (with_lcp && e) {
                        const uint32_t sp = perm[e - 1];
                        if (SLOTREC) l = slot_pair_lcp<BITS, idx_t>(P, n, (uint64_t)skey[sp], ssa[sp], (uint64_t)key, sa, tie_from);
                        else l = TILE_EMIT_LCP_(skey[sp], ssa[sp], key, sa);
                    }
                    if (direct) {
                        STREAM_STORE(&fin.sa[start + e], sa);
                        STREAM_STORE(&fin.lcp[start + e], (idx_t)l);
                        if (e == 0) { fin.first_key[g] = key; fin.first_sa[g] = sa; }
                        if (e == cnt - 1) { fin.last_key[g] = key; fin.last_sa[g] = sa; }
                    } else {
                        out_key[start + e] = key;
                        out_sa[start + e] = sa;
                        if (with_lcp) out_lcp[start + e] = (idx_t)l;
                    }
                }
            }
        }
    } else {
        TILE_SORT_EMIT
    }
    PHASE_MARK(6);                                             // emit (+ LCPs); the stores themselves drain after the mark
}

// The tile table for the kernels at the head of the queue chain of a sort over slots with outgrown buckets (tile_sort_kernel, the start of a tile):
// a copy in which the tiles of every segment longer than slot_cap are empty.
GLOBAL_FN LAUNCH_BOUNDS(256) hot_tiles_kernel(KCTX SegDesc sd, uint32_t slot_cap, TileInfo* __restrict__ hot)
{
    PAR(tid) {
        const uint32_t nt = sd.tile_off[sd.G];
        const uint32_t i = K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (i < nt) {
            TileInfo t = sd.tile_rec[i];
            if (t.s1 - t.s0 > (uint64_t)slot_cap) { t.s1 = t.s0; t.tl = 0; }
            hot[i] = t;
        }
    }
}

// Every tile straight into tile_sort_kernel's queue of unfinished tiles (skewed keys, pipeline.h SortOpts::skewed_keys:
// the linear bin map would crowd nearly every tile -- 97 % of a genome-like text's -- and its attempt is then pure cost).
GLOBAL_FN LAUNCH_BOUNDS(256) queue_all_tiles_kernel(KCTX SegDesc sd, uint32_t* __restrict__ redo)
{
    PAR(tid) {
        const uint32_t nt = sd.tile_off[sd.G];
        const uint32_t i = K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (i < nt) redo[1 + i] = i;
        if (i == 0) redo[0] = nt;
    }
}

// Slots of 8-byte records (tile_sort_kernel SLOTREC): the kernels behind tile_sort_kernel in the queue chain read an index array and cut
// their 64-bit keys from the text (their keys_from_text route, as behind 32-bit keys).  The indices of the QUEUED tiles -- a handful,
// none on random DNA -- are copied out of their records into the index array of the two-array view of the slots, which lies behind the
// records and is idle: no record layout in the three large kernels.  A fixed grid walks the queue.
GLOBAL_FN LAUNCH_BOUNDS(256) slot_unpack_kernel(KCTX SegDesc sd, const uint32_t* __restrict__ redo, uint32_t slot_cap,
                                                const uint64_t* __restrict__ rec, uint32_t* __restrict__ out_sa)
{
    const uint32_t n_redo = redo[0];
    for (uint32_t qi = K_BLOCK_IDX; qi < n_redo; qi += K_GRID_DIM) {
        const TileInfo t = tile_info(sd, redo[1 + qi]);
        const uint64_t len = t.s1 - t.s0, in0 = (uint64_t)t.g * slot_cap;
        const uint32_t cnt = (uint32_t)(len < slot_cap ? len : slot_cap);
        PAR(tid) {
            for (uint32_t i = tid; i < cnt; i += K_BLOCK_DIM) out_sa[in0 + i] = (uint32_t)(rec[in0 + i] >> 32);
        }
    }
}

// CAPS_SA_DEBUG only, behind a sort over slots of slot-key records: count[0] = neighbours of the result inside one bucket whose
// slot keys were equal (their keys agree above the bucket's shift) -- the pairs the tile sort had to settle from the text;
// count[1] = bucket heads whose key agrees above the shift with the key of the element before them (the last one of the bucket
// below): ties ACROSS a boundary, whose LCP head_lcp_kernel must take from the text.
template <typename idx_t, int BITS>
GLOBAL_FN LAUNCH_BOUNDS(256) slot_tie_count_kernel(KCTX const uint32_t* __restrict__ P, const uint64_t* __restrict__ seg_start, uint32_t G,
                                                   const uint8_t* __restrict__ kshift, const idx_t* __restrict__ sa,
                                                   uint64_t* __restrict__ count)
{
    for (uint32_t g = K_BLOCK_IDX; g < G; g += K_GRID_DIM) {
        const uint64_t s0 = seg_start[g], s1 = seg_start[g + 1];
        const uint32_t s = kshift[g];
        PAR(tid) {
            uint64_t c = 0;
            for (uint64_t i = s0 + 1 + tid; i < s1; i += K_BLOCK_DIM)
                c += (window64<BITS>(P, (uint64_t)sa[i - 1]) >> s) == (window64<BITS>(P, (uint64_t)sa[i]) >> s) ? 1u : 0u;
            if (c) ATOMIC_ADD_U64(count, c);
            if (tid == 0 && s1 > s0 && s0 > 0 && (window64<BITS>(P, (uint64_t)sa[s0 - 1]) >> s) == (window64<BITS>(P, (uint64_t)sa[s0]) >> s))
                ATOMIC_ADD_U64(count + 1, 1ull);
        }
    }
}

// ---- tile_sort_eq_kernel: second chance for the tiles tile_sort_kernel could not finish --------
// Keys that are far from uniform over the tile's range (skewed k-mer composition: every real genome)
// crowd a few bins of the linear map.  Here the map is equalised with the tile's own data, iteratively:
// every element holds a 24-bit POSITION (bin.fraction, first from the linear map); the histogram of the
// positions' bins is a piecewise-linear CDF, and the new position is the estimated rank it gives:
// (count before my bin + fraction x count of my bin) * TILE_BINS / cnt.  After EQ_ROUNDS rounds the bin of
// the position is the counting sort's bin -- monotone in the key, so the exact in-bin ranking of tile_sort_kernel
// finish the job unchanged.  Takes the tiles from tile_sort_kernel's queue (redo[0] = length), with a fixed grid or one
// workgroup per entry (PERSIST below); a tile that still has a bin above TILE_BIN_LIMIT (clusters of suffixes that share more
// chars than the coarse bins resolve), or a deep tie, goes on to tile_sort_general_kernel (redo2).
// A separate kernel rather than a branch of tile_sort_kernel: that one runs at the register budget.
#ifndef CAPS_EQ_ROUNDS
#define CAPS_EQ_ROUNDS 2          /* measured on skewed-Markov tiles (simulation): largest bin, median 243 (linear) -> 50 / 26 / 13 after 1 / 2 / 3 rounds */
#endif
constexpr uint32_t EQ_ROUNDS = CAPS_EQ_ROUNDS;
#ifndef CAPS_TIE_G1
#define CAPS_TIE_G1 8
#endif
#ifndef CAPS_TIE_LIST_MAX
#define CAPS_TIE_LIST_MAX 2       /* g3 / g3r / g2r at 1, 2, 3, 6, 12: 97.9 98.2 98.4 99.9 100.1 / 150.7 150.5 151.7 153.0 - / 17.8 17.9 17.5 18.5 18.4 ms (beyond: phase B) */
#endif
constexpr uint32_t TIE_G1 = CAPS_TIE_G1;          // lanes (= windows) per listed tie in the first round,
constexpr uint32_t TIE_G2 = 64;                   //   per tie that is still equal in the second
constexpr uint32_t TIE_LIST_CAP = TILE_E / 8;     // list entries per tile (pairs from the bottom, elements' own entries from the top)
constexpr uint32_t TIE_LIST_MAX = CAPS_TIE_LIST_MAX;   // an element lists up to this many equal keys (more: it scans them itself)
constexpr uint32_t TIE_DEEP_CAP = 64;             // entries that may go to the second round
constexpr uint32_t TIE_VDEEP_CAP = 32;            //   ... and on to the third (any depth: long exact duplicates)
constexpr uint32_t TIE_BIG_CAP = 1024;            // elements with more than TIE_LIST_MAX equal keys a tile may hold
constexpr uint32_t TIE_BIG_LANES = 64;            //   lanes that share the equal keys of one of them (fewer when there are many)
constexpr uint32_t EQ_FRAC_BITS = 13;             // position inside a bin; a position is bin * 2^13 + fraction < 2^24 at 2048 bins
static_assert((uint64_t)TILE_BINS_ << EQ_FRAC_BITS <= (1u << 24), "positions fit 24 bits");

// Position of the key on the tile's linear map: (bin of bucket_of(tb, .)) << EQ_FRAC_BITS plus that many more bits
DEV_INLINE uint32_t eq_pos(const BucketParams& bp, uint64_t key)
{
    const uint32_t top = (bp.B << EQ_FRAC_BITS) - 1u;
    if (key <= bp.kmin) return 0;
    const uint64_t d = key - bp.kmin;
    if (d >= bp.range) return top;
    const uint32_t d32 = (uint32_t)((d << bp.shift) >> 32);
    const uint64_t prod = (uint64_t)d32 * bp.m;
    const uint32_t sh = 32u + bp.post;                                   // bucket = prod >> sh
    const uint32_t x = (uint32_t)(sh >= EQ_FRAC_BITS ? prod >> (sh - EQ_FRAC_BITS) : prod << (EQ_FRAC_BITS - sh));
    return x < top ? x : top;
}

// the lcp noted for slot e in the table of the few lcps beyond 15 bits (0: not there -- the caller derives it from the text)
DEV_INLINE uint32_t eq_big_lcp(const uint16_t* vslot, const uint32_t* vlcp, uint32_t cnt, uint32_t e)
{
    uint32_t l = 0;
    for (uint32_t q = 0; q < cnt && q < TIE_VDEEP_CAP; ++q)
        if (vslot[q] == e) l = vlcp[q];
    return l;
}

// lcp of two neighbours of the sorted tile that no tie has settled.  TEXT = false (the plain build): their keys differ --
// every pair of equal keys has its lcp from the tie phases, and those are never 0 -- so the keys tell; the comparator through
// the text, unrolled four times in the emit phase, cost that phase registers (scratch) for a path no tile takes.
template <int BITS, bool TEXT, typename idx_t>
DEV_INLINE uint64_t eq_emit_lcp(const uint32_t* __restrict__ P, uint64_t n, uint64_t ka, idx_t a, uint64_t kb, idx_t b, uint32_t* lost, bool test_drop)
{
    if (TEXT) return pair_lcp<BITS, false>(P, n, ka, (uint64_t)a, kb, (uint64_t)b);
    const uint64_t x = ka ^ kb;
    if (x == 0) {
        // The invariant the plain build rests on: equal keys always come with their lcp from the tie phases.  Should a note ever be
        // lost, the capped key length would be a WRONG lcp: the tile is handed to the comparison sort instead (*lost, read by the
        // kernel behind its last barrier), which sorts it again from its input.  The emulation aborts (unless the test switch that
        // drops notes on purpose is on): there the invariant is a test.
#ifdef CAPS_EMUL
        if (!test_drop) { std::fprintf(stderr, "eq_emit_lcp: neighbours %llu, %llu with equal keys and no lcp from the tie phases\n", (unsigned long long)a, (unsigned long long)b); std::abort(); }
#endif
        *lost = 1;                                                   // (benign race: every writer stores 1)
    }
    return lcp_capped<idx_t>(x ? (uint32_t)caps_clz64(x) / BITS : TextTraits<BITS>::KCH, n, a, b);
}

#ifndef CAPS_EQ_WAVES
#define CAPS_EQ_WAVES TILE_WAVES_PER_SIMD
#endif
#undef TILE_EMIT_LCP_
#define TILE_EMIT_LCP_(ka, a, kb, b) eq_emit_lcp<BITS, VDEEP>(P, n, ka, a, kb, b, &flag[1], TEST_DROP)
#undef TILE_SRC_KEY
#undef TILE_SRC_SA
#define TILE_SRC_KEY src_key
#define TILE_SRC_SA src_sa
#ifndef CAPS_EQ_FULL_SYNC          /* measurement: -DCAPS_EQ_FULL_SYNC keeps __syncthreads() in this kernel */
#undef TILE_SYNC
#define TILE_SYNC() SYNC_LDS()
#endif
// this kernel and tile_sort_general_kernel: every PAR region takes its thread index afresh (kernel_lang.h PAR_FRESH; measured
// at 3e9 genome-like: 57.3 -> 54.1 ms here, no register left in scratch)
#if !defined(CAPS_EMUL) && !defined(CAPS_PAR_PLAIN_ONLY)
#pragma push_macro("PAR")
#undef PAR
#define PAR(tid) PAR_FRESH(tid)
#define CAPS_PAR_SWITCHED
#endif
// VDEEP: the build with the third tie stage (any depth).  A build of its own, behind the plain one in the queue chain: the
// plain kernel runs at the register budget, and the stage's code in it cost every tile of a genome-like text 14 % (76 -> 87 ms
// at 3e9) for the sake of the few that hold an exact long duplicate.
// PERSIST = false: one queue entry per workgroup (the grid covers the queue: the caller knows its length, or a bound).  The
// loop over the queue lets the compiler hoist per-thread addresses and constants out of it, and what it hoists it must hold
// across all ~20 phases of a tile: at the 64-register budget that put 41 registers in scratch memory, reloaded 58 times per
// tile (and 13 GB of scratch stores reached HBM at 3e9); without the loop: 11, reloaded 5 times, 19 % fewer instructions.
template <typename idx_t, int BITS, bool FROM_TEXT, bool VDEEP = false, bool PERSIST = true>
GLOBAL_FN LAUNCH_BOUNDS2(TILE_NT, CAPS_EQ_WAVES) tile_sort_eq_kernel(KCTX SegDesc sd, const uint32_t* __restrict__ P, uint64_t n,
                                                  uint64_t text_base, uint32_t lcp_mode, uint32_t slot_cap, const uint64_t* in_key,
                                                  const idx_t* in_sa, uint64_t* out_key, idx_t* out_sa, idx_t* out_lcp,
                                                  FinalOut<idx_t> fin, const BucketParams* __restrict__ seg_map,
                                                  const uint32_t* __restrict__ redo, uint32_t* __restrict__ redo2, uint32_t keys_from_text,
                                                  uint32_t* __restrict__ redo_deep)
{
    // redo_deep (the plain build): the queue of the tiles whose ONLY obstacle was a tie deeper than the first two rounds see -- the
    // VDEEP build's; everything else this kernel cannot finish goes to redo2, the comparison sort's
    // keys_from_text != 0: the slots hold 32-bit keys (tile_sort_kernel<..., uint32_t> ran first); this kernel works on the
    // 64-bit keys, cut from the text at the elements' positions (seg_map is then null: the tile's own key range)
    constexpr bool TILE_RUNS = false;
    const bool TILE_KEYS_FROM_TEXT = (keys_from_text & 1u) != 0;
    // bit 1 of keys_from_text (tests only, CAPS_SA_TEST_DROP_NOTE): the lcp notes of tied pairs are dropped on purpose -- the emit
    // phase must then notice equal keys without a note and hand the tile to the comparison sort (eq_emit_lcp)
    const bool TEST_DROP = (keys_from_text & 2u) != 0;
    const uint32_t TILE_KEY_SHIFT = 0;
    (void)TILE_RUNS;
    (void)TILE_KEY_SHIFT;
    SHARED_ARRAY(uint64_t, skey, TILE_E);
    SHARED_ARRAY(idx_t, ssa, TILE_E);
    SHARED_ARRAY(uint32_t, hist, TILE_BINS + 1);
    // 32-bit indices: 80 KB of LDS with these two (two workgroups per CU); 64-bit indices have no room for sbin, and a shorter list
    constexpr bool SLOT_ORDER = sizeof(idx_t) == 4;
    constexpr uint32_t BIG_CAP = sizeof(idx_t) == 4 ? TIE_BIG_CAP : TIE_BIG_CAP / 4;
    SHARED_ARRAY(uint16_t, sbin, SLOT_ORDER ? TILE_E : 1);   // the bin of the element in slot e (after the placement by bin)
    // PERM (where sbin exists): no second placement.  Once an element knows its final position d it only notes perm[d] = its slot (in
    // sbin's memory, dead by then) and leaves its lcp note in tinfo[slot]; the emit phase reads keys and indices THROUGH perm.  The
    // pick-up of (key, index) into registers, the barrier, their second trip through LDS and the registers they held are gone.
    constexpr bool PERM = SLOT_ORDER;
    uint16_t* perm = sbin;
    SHARED_ARRAY(uint64_t, kmm, 2);
    SHARED_ARRAY(uint32_t, flag, 2);         // [0] the tile is the comparison sort's; [1] it only needs the third tie stage; during the
                                             //   emit phase [1]: neighbours with equal keys and no lcp note (eq_emit_lcp)
    TL_DECL(uint64_t, rk, TILE_EPT);
    TL_DECL(idx_t, rs, TILE_EPT);
    TL_DECL(uint32_t, rd, TILE_EPT);
    TL_DECL(uint32_t, rb, TILE_EPT);
    TL_DECL(uint32_t, rt, TILE_EPT);         // rank phase: rank inside the bin | first own entry << 8 | ties << 28
    TL_DECL(uint32_t, rl, TILE_EPT);         // lcp with the predecessor where a tie settled it
    TL_DECL(uint64_t, twa, 1);               // tie rounds: the lane's pair of windows,
    TL_DECL(uint64_t, twb, 1);
    TL_DECL(uint32_t, tpi, 1);               //   its entry (index | own-entry flag << 31 | virtual index << 16; ~0: none)
    SHARED_ARRAY(uint32_t, plist, TIE_LIST_CAP);      // ties: first differing window << 24 | slot << 12 | the other's slot;
                                                      //   an own entry once settled: 0x80 | the other sorts first, << 24 | lcp
    SHARED_ARRAY(uint16_t, deep, TIE_DEEP_CAP);       // entries (virtual index) still equal after the first round
    SHARED_ARRAY(uint16_t, vdeep, TIE_VDEEP_CAP);     //   ... and after the second: settled one by one, the whole workgroup on each
    SHARED_ARRAY(uint32_t, pcnt, 8);                  // pairs listed, own entries listed, entries on `deep`, on `vdeep`, [4] first hit, [5] big lcps,
                                                      //   [6] elements on `big`
    SHARED_ARRAY(uint32_t, big, BIG_CAP);             // elements with more than TIE_LIST_MAX equal keys: slot | first of bin << 12 | bin size - 1 << 24
    SHARED_ARRAY(uint32_t, bmore, BIG_CAP);           //   how many of its equal keys sort before it,
    SHARED_ARRAY(uint32_t, bbest, BIG_CAP);           //   the largest lcp with one of those
    SHARED_ARRAY(uint32_t, vlcp, TIE_VDEEP_CAP);      // third stage: the lcp of pair q (too large for the 15 bits of its members' notes);
                                                      //   after the final placement: the lcps >= 0x7FFF, with ...
    SHARED_ARRAY(uint16_t, vslot, TIE_VDEEP_CAP);     //   ... the slots they belong to
    SHARED_ARRAY(uint32_t, vlcp2, PERM ? TIE_VDEEP_CAP : 1);   // PERM: the lcps >= 0x7FFF live here (vlcp is still being read when they are noted)
    static_assert((TILE_BINS + 1) * sizeof(uint32_t) >= TILE_E * sizeof(uint16_t) && TILE_E <= (1u << 12) && EQ_BIN_LIMIT <= 128 &&
                  TILE_NT % TIE_G1 == 0 && TILE_NT % TIE_G2 == 0 && TIE_G1 + TIE_G2 < 0x80u && TIE_LIST_CAP <= (1u << 12) &&
                  TIE_BIG_CAP <= (1u << 12) && (TILE_NT & (TILE_NT - 1u)) == 0 &&
                  TextTraits<BITS>::KCH * (1u + TIE_G1 + TIE_G2) < 0x7FFFu,
                  "tinfo fits hist; slots and entries fit 12 bits; ranks inside a bin fit 8 bits; lcps of the first two rounds fit 15 bits");
    // per slot: "the other member of my pair sorts before me" << 15 | their lcp (0x7FFF: see vlcp); after the final placement: the
    // lcp with the predecessor where a tie settled it (0x7FFF: see vslot / vlcp)
    uint16_t* tinfo = reinterpret_cast<uint16_t*>(hist);
    // redo == nullptr (PERSIST = false only): every tile is this kernel's and the grid is the tile count -- no queue to read (one
    // dependent round trip to memory less at the head of every tile)
    const uint32_t n_redo = redo ? redo[0] : K_GRID_DIM;
    PAR_TID_DECL;
    // (fetching the queue entry and the record of the NEXT tile while this one is sorted was tried: no gain, and the record's
    // registers, held across the whole tile, went to scratch)
    uint32_t qi = K_BLOCK_IDX;
    if (qi >= n_redo) return;
    do {
    PAR_TID_RESET;
    const uint32_t b = redo ? redo[1 + qi] : qi;
    if (!EQ_OK(b < sd.tile_off[sd.G], 0)) return;
    const TileInfo t = tile_info(sd, b);
    const uint32_t g = t.g;
    const uint64_t start = t.s0 + (uint64_t)t.tl * TILE_E;
    if (!EQ_OK(g < sd.G && t.s0 <= start && start < t.s1, 1)) return;
    const uint32_t cnt = (uint32_t)(t.s1 - start < TILE_E ? t.s1 - start : TILE_E);
    const bool with_lcp = lcp_mode != 0 && (t.s1 - t.s0) <= TILE_E;
    const bool direct = with_lcp && fin.sa != nullptr;
    // a bucket that outgrew its slot (tile_sort_kernel, the start of a tile): the plain build sees its tiles empty and passes them on (`fast` below is
    // false for them, no flag is up: redo_deep); the VDEEP build reads them where they were put together -- at their place in the
    // output arrays -- and sorts them in place
    const bool in_slot = !VDEEP || !TILE_OUTGROWN;
    const uint64_t in0 = slot_cap != 0 && in_slot ? (uint64_t)g * slot_cap : start;
    const uint64_t* src_key = tile_src(in_key, out_key, !in_slot);
    const idx_t* src_sa = in_slot ? in_sa : out_sa;
    PHASE_T0();
    TILE_SORT_LOAD
#if defined(CAPS_EQ_CHECK) && !defined(CAPS_EMUL)
    PAR(tid) { for (uint32_t k = 0; k < TILE_EPT; ++k) if (tid + k * TILE_NT < cnt) EQ_CHK((uint64_t)TL(rs, tid, k) < n || n == 0, 2); }
#endif
    TILE_SORT_RANGE
    PHASE_MARK(8);                                             // load
    bool fast = cnt > EQ_BIN_LIMIT && tb.range > 0 && tb.B == TILE_BINS;
    if (fast) {
        PAR_FRESH_SET(tid) {
            UNROLL
            for (uint32_t k = 0; k < TILE_EPT; ++k) {
                const uint32_t e = tid + k * TILE_NT;
                if (e < cnt) TL(rb, tid, k) = eq_pos(tb, TL(rk, tid, k));
            }
        }
        // position -> estimated rank, EQ_ROUNDS times: histogram of the positions' bins, its prefix sums are a
        // piecewise-linear CDF, the new position is the CDF value scaled back to [0, TILE_BINS)
        // estimated rank -> position: E * TILE_BINS / cnt.  In single precision: only monotony in E counts (equal or larger E
        // never gives a smaller position: conversion, product and truncation are all monotone), and E < 2^27, so the 64-bit
        // product this used to be cost three times the instructions for bits the bins never see.
        const float Kf = (float)TILE_BINS / (float)cnt;
        for (uint32_t round = 0; round < EQ_ROUNDS; ++round) {
            if (round) {
                PAR_SAME_G(1a, tid) { for (uint32_t i = tid; i <= TILE_BINS; i += K_BLOCK_DIM) hist[i] = 0; }
                TILE_SYNC();
            }
            PAR_SAME_G(1b, tid) {
                UNROLL
                for (uint32_t k = 0; k < TILE_EPT; ++k) {
                    const uint32_t e = tid + k * TILE_NT;
                    if (e < cnt && EQ_OK((TL(rb, tid, k) >> EQ_FRAC_BITS) < TILE_BINS, 3)) FETCH_ADD_U32(&hist[TL(rb, tid, k) >> EQ_FRAC_BITS], 1u);
                }
            }
            TILE_SYNC();
            block_exclusive_scan_bins(KCTX_PASS hist);
            PAR_SAME_G(1c, tid) {
                UNROLL
                for (uint32_t k = 0; k < TILE_EPT; ++k) {
                    const uint32_t e = tid + k * TILE_NT;
                    if (e < cnt) {
                        const uint32_t x = TL(rb, tid, k);
                        const uint32_t bn = x >> EQ_FRAC_BITS, fr = x & ((1u << EQ_FRAC_BITS) - 1u);
                        EQ_CHK(bn < TILE_BINS, 4);
                        const uint32_t before = hist[bn], here = hist[bn + 1] - before;
                        const uint32_t E = (before << EQ_FRAC_BITS) + here * fr;                          // < cnt * 2^13 <= 2^25 (+ 2^25)
                        const uint32_t y = (uint32_t)((float)E * Kf);                                     // ~ E * TILE_BINS / cnt
                        TL(rb, tid, k) = y < (TILE_BINS << EQ_FRAC_BITS) ? y : (TILE_BINS << EQ_FRAC_BITS) - 1u;
                    }
                }
            }
            TILE_SYNC();
        }
        PHASE_MARK(9);                                         // equalisation rounds
        PAR_SAME_G(1d, tid) {
            for (uint32_t i = tid; i <= TILE_BINS; i += K_BLOCK_DIM) hist[i] = 0;
            if (tid < 8) pcnt[tid] = 0;
            if (tid == 0) flag[1] = 0;
            for (uint32_t i = tid; i < BIG_CAP; i += K_BLOCK_DIM) { bmore[i] = 0; bbest[i] = 0; }
        }
        TILE_SYNC();
        PAR_SAME_G(1e, tid) {
            UNROLL
            for (uint32_t k = 0; k < TILE_EPT; ++k) {
                const uint32_t e = tid + k * TILE_NT;
                if (e < cnt) {
                    const uint32_t bin = TL(rb, tid, k) >> EQ_FRAC_BITS;
                    EQ_CHK(bin < TILE_BINS, 5);
                    const uint32_t r = FETCH_ADD_U32(&hist[bin], 1u);
                    if (r >= EQ_BIN_LIMIT) flag[0] = 1;
                    TL(rb, tid, k) = bin;
                    TL(rd, tid, k) = r;
                }
            }
        }
        TILE_SYNC();
        fast = flag[0] == 0;
        PHASE_MARK(10);                                        // final histogram
    }
    if (fast) {                                                // from here on: as in tile_sort_kernel
        block_exclusive_scan_bins(KCTX_PASS hist);
        PHASE_MARK(11);                                        // scan
        PAR_SAME_G(1f, tid) {
            UNROLL
            for (uint32_t k = 0; k < TILE_EPT; ++k) {
                const uint32_t e = tid + k * TILE_NT;
                if (e < cnt) {
                    const uint32_t slot = hist[TL(rb, tid, k)] + TL(rd, tid, k);
                    if (!EQ_OK(slot < cnt, 6)) continue;
                    skey[slot] = TL(rk, tid, k);
                    ssa[slot] = TL(rs, tid, k);
                    if (SLOT_ORDER) sbin[slot] = (uint16_t)TL(rb, tid, k);
                    else TL(rd, tid, k) = slot;
                }
            }
        }
        TILE_SYNC();
        PHASE_MARK(12);                                        // place by bin
        // ---- exact rank inside the bin.  Ties (equal keys: 2 % of a genome-like text's neighbours, repeats with a
        // mutation every ~100 chars) need the text, several windows deep, every window a dependent HBM read of ~1 us.  Inside
        // the ranking loop such a read stalls the whole wave once per tie and window, one after the other: measured with the
        // phase clock (tools/phase_clock.py), 53 % of this kernel's time, and 24 % more in the emit phase, which read the same
        // text again for the lcps.  So:
        //  R1  rank by keys only and note the ties.  A PAIR of equal keys (91 % of the tied elements of a genome-like text) is
        //      listed once, by its member with the higher slot; an element with 2 .. TIE_LIST_MAX equal keys lists (itself, the
        //      other) for each of them -- its own entries, from the top of the same list;
        //  T   the workgroup settles the listed entries together, several lanes per entry, one window each, all loads of a
        //      round in flight at once: TIE_G1 windows deep for ONE memory latency.  The lane with the first difference (an
        //      LDS atomic min on the entry) derives order and lcp: for a pair it leaves them for both members in tinfo, for
        //      an own entry in the entry itself.  What is still equal (one tie in eight on such a text) goes on a short list
        //      and gets TIE_G2 lanes per entry in a second round; still equal after that (TIE_G1 + TIE_G2 windows), or more
        //      ties than the lists hold: the tile is the comparison sort's;
        //  B   an element with more than TIE_LIST_MAX equal keys: its own lanes, one comparison each (below);
        //  R3  the elements pick their outcomes up.
        // The lcp of an element with its predecessor in the final order is the largest lcp with a smaller member of its tie
        // group; it travels with the element to its final slot (slcp) and the emit phase uses it instead of the text.
        // tinfo / slcp: u16 per slot, in the memory of hist (free once R1 has read the bin bounds).
        PAR(tid) {
            UNROLL
            for (uint32_t k = 0; k < TILE_EPT; ++k) {
                const uint32_t e = tid + k * TILE_NT;
                if (e < cnt) {
                    // from here on a thread works on the elements in SLOTS tid + k * TILE_NT (the slot's bin: sbin), not on the
                    // ones it loaded: the lanes of a wave then hold neighbouring slots -- mostly one bin, so they scan the same
                    // keys (one LDS read serves them all) for the same number of steps, where the lanes of a wave used to sit
                    // in 64 bins of 64 sizes.  The elements live in skey / ssa only until the final placement.
                    // (64-bit indices: no room in LDS for sbin; every thread stays with the elements it loaded)
                    const uint32_t slot = SLOT_ORDER ? e : TL(rd, tid, k), bin = SLOT_ORDER ? (uint32_t)sbin[slot] : TL(rb, tid, k);
                    TL(rd, tid, k) = slot;
                    EQ_CHK(bin < TILE_BINS && slot < cnt, 7);
                    const uint32_t bs = hist[bin], be = hist[bin + 1];
                    EQ_CHK(bs <= slot && slot < be && be <= cnt && be - bs <= EQ_BIN_LIMIT, 8);
                    const uint64_t key = skey[slot];
                    uint32_t less = 0, ties = 0, tj = 0;
                    for (uint32_t j = bs; j < be; ++j) {
                        const uint64_t kj = skey[j];
                        less += kj < key ? 1u : 0u;
                        if (kj == key && j != slot) { ++ties; tj = j; }
                    }
                    uint32_t own = 0;                                      // my first entry, counted from the top of the list
                    if (ties == 1u && slot > tj) {
                        const uint32_t pi = FETCH_ADD_U32(&pcnt[0], 1u);
                        // (RACY_STORE: pairs from the bottom and own entries from the top run into each other only when np + nm >
                        // TIE_LIST_CAP, and then the tile fails below before anything reads the list)
                        if (pi < TIE_LIST_CAP) RACY_STORE_U32(&plist[pi], 0xFF000000u | (slot << 12) | tj);
                    } else if (ties >= 2u && ties <= TIE_LIST_MAX) {
                        own = FETCH_ADD_U32(&pcnt[1], ties);
                        if (own + ties <= TIE_LIST_CAP) {
                            uint32_t q = own;
                            for (uint32_t j = bs; j < be; ++j)
                                if (skey[j] == key && j != slot) RACY_STORE_U32(&plist[TIE_LIST_CAP - 1u - q++], 0xFF000000u | (slot << 12) | j);
                        } else {
                            own = 0;                                       // (the tile fails below: the list is full)
                        }
                    } else if (ties > TIE_LIST_MAX) {
                        own = FETCH_ADD_U32(&pcnt[6], 1u);                 // here: my place on `big`
                        if (own < BIG_CAP) big[own] = slot | (bs << 12) | ((be - bs - 1u) << 24);
                        else { own = 0; flag[0] = 1; }                     // (more such elements than the list holds: not here)
                    }
                    TL(rb, tid, k) = bs | (be << 16);                      // the bin id is not needed any more
                    TL(rt, tid, k) = less | (own << 8) | (ties > 15u ? 15u << 28 : ties << 28);   // less <= 127, own < 2^12
                }
            }
        }
        TILE_SYNC();                                                // hist is free: tinfo / slcp from here on
        PHASE_MARK(16);                                        // R1: rank by keys
        // B: the elements with more than TIE_LIST_MAX equal keys (0.1 % of a genome-like text's suffixes, in clusters: every
        // tenth tile holds some).  Each gets up to TIE_BIG_LANES lanes that share its bin: every lane compares it with its share
        // of the equal keys through the text, the comparisons of an element in flight at once -- in the pick-up phase, where every such element
        // went through its equal keys one after the other (c - 1 dependent trips to the text for each member of a cluster of
        // c), the whole workgroup waited for the longest chain, and the comparator's code, unrolled there four times, put
        // that phase on scratch memory.
        {
            const uint32_t nb = pcnt[6] < BIG_CAP ? pcnt[6] : BIG_CAP;                     // block-uniform
            uint32_t lg = 0;                                                               // lanes per element: 2^lg <= TIE_BIG_LANES,
            while ((2u << lg) <= TIE_BIG_LANES && (uint64_t)nb * (2u << lg) <= TILE_NT) ++lg;   //   as many as one round has room for
            for (uint32_t base = 0; base < nb; base += TILE_NT >> lg) {
                PAR(tid) {
                    const uint32_t i = base + (tid >> lg);
                    if (i < nb) {
                        const uint32_t ent = big[i], slot = ent & 0xFFFu, bs = (ent >> 12) & 0xFFFu, be = bs + (ent >> 24) + 1u;
                        EQ_CHK(slot < cnt && be <= cnt, 9);
                        const uint64_t key = skey[slot];
                        const uint64_t sa = (uint64_t)ssa[slot];
                        uint32_t more = 0, best = 0;
                        for (uint32_t j = bs + (tid & ((1u << lg) - 1u)); j < be; j += 1u << lg) {
                            if (skey[j] == key && j != slot) {
                                uint32_t l;
                                const uint32_t c = tie_order_lcp_bounded<BITS>(P, n, (uint64_t)ssa[j], sa, l);   // 1: j sorts before me
                                if (c == 2u) flag[0] = 1;
                                if (c == 1u) { ++more; best = l > best ? l : best; }
                            }
                        }
                        if (more) { FETCH_ADD_U32(&bmore[i], more); ATOMIC_MAX_U32(&bbest[i], best); }
                    }
                }
            }
        }
        PHASE_MARK(18);                                        // B: elements with many equal keys
        {
            const uint32_t np = pcnt[0], nm = pcnt[1];                                     // block-uniform
            constexpr uint32_t KCH_ = TextTraits<BITS>::KCH;
            if (np + nm > TIE_LIST_CAP) {
                PAR(tid) { if (tid == 0) flag[0] = 1; }                                    // more ties than the list holds: not here
            } else if (np + nm) {
                for (uint32_t round = 0; round < 2; ++round) {
                    // round 0: every entry, TIE_G1 lanes each; round 1: the entries on the short list, TIE_G2 lanes each
                    const uint32_t G = round ? TIE_G2 : TIE_G1, W0 = round ? TIE_G1 : 0u;
                    const uint32_t n_ent = round ? (pcnt[2] < TIE_DEEP_CAP ? pcnt[2] : TIE_DEEP_CAP) : np + nm;
                    if (round && pcnt[2] > TIE_DEEP_CAP) { PAR(tid) { if (tid == 0) flag[0] = 1; } }
                    for (uint32_t base = 0; base < n_ent; base += TILE_NT / G) {
                        PAR_FRESH_SET(tid) {
                            const uint32_t vi = base + tid / G, W = W0 + tid % G;
                            TL(twa, tid, 0) = 0;
                            TL(twb, tid, 0) = 0;
                            TL(tpi, tid, 0) = ~0u;
                            if (vi < n_ent) {
                                const uint32_t vj = round ? deep[vi] : vi;
                                const uint32_t pi = vj < np ? vj : TIE_LIST_CAP - 1u - (vj - np);
                                const uint32_t ent = RACY_LOAD_U32(&plist[pi]);     // (the lanes of this entry may have touched it: below)
                                TL(tpi, tid, 0) = pi | (vj < np ? 0u : 0x80000000u) | (vj << 16);
                                // open: untouched (0xFF) or touched by another lane of THIS round (its window number) -- not
                                // "untouched" alone: the lanes of an entry would then depend on each other's timing (they do run
                                // in lockstep, one wave holds them all, but nothing here should need that; the reversed-order
                                // emulation, tests/test_emul_pipeline.py, found it)
                                const uint32_t tb = ent >> 24;
                                if (tb == 0xFFu || (tb >= W0 && tb < W0 + G)) {
                                    EQ_CHK((ent & 0xFFFu) < cnt && ((ent >> 12) & 0xFFFu) < cnt, 10);
                                    const uint64_t a = (uint64_t)ssa[ent & 0xFFFu], b2 = (uint64_t)ssa[(ent >> 12) & 0xFFFu];
                                    EQ_CHK(a < n && b2 < n, 11);
                                    const uint64_t maxlen = a < n && b2 < n ? n - (a > b2 ? a : b2) : 0;   // corrupt index: settle at once
                                    const uint64_t l = (uint64_t)KCH_ * (1u + W);
                                    bool hit = l >= maxlen;               // the shorter suffix ends before this window
                                    if (!hit) {
                                        const uint64_t wa = window64<BITS>(P, a + l), wb = window64<BITS>(P, b2 + l);
                                        TL(twa, tid, 0) = wa;
                                        TL(twb, tid, 0) = wb;
                                        hit = wa != wb;
                                    }
                                    if (hit) ATOMIC_MIN_U32(&plist[pi], (W << 24) | (ent & 0xFFFFFFu));
                                }
                            }
                        }
                        TILE_SYNC();
                        PAR_SAME_G(2, tid) {
                            const uint32_t W = W0 + tid % G, tp = TL(tpi, tid, 0);
                            if (tp != ~0u) {
                                const uint32_t pi = tp & 0xFFFFu, vj = (tp >> 16) & 0x7FFFu;
                                // (racing with the winner's store below by design: a settled own entry reads 0x80 / 0x81 in its top byte,
                                // which is neither a window number nor 0xFF, and the lane that reads it does nothing)
                                const uint32_t ent = RACY_LOAD_U32(&plist[pi]), lo = ent & 0xFFFu, hi = (ent >> 12) & 0xFFFu;
                                if ((ent >> 24) == W) {                   // mine is the first window that differs (or ends)
                                    const uint64_t a = (uint64_t)ssa[lo], b2 = (uint64_t)ssa[hi];
                                    const uint64_t maxlen = a < n && b2 < n ? n - (a > b2 ? a : b2) : 0;
                                    const uint64_t l = (uint64_t)KCH_ * (1u + W);
                                    const uint64_t wa = TL(twa, tid, 0), wb = TL(twb, tid, 0);
                                    uint64_t d = maxlen;
                                    bool lo_first = a > b2;               // one is a prefix of the other: the shorter first
                                    if (l < maxlen) {
                                        d = l + (uint32_t)caps_clz64(wa ^ wb) / BITS;
                                        d = d < maxlen ? d : maxlen;
                                        lo_first = wa < wb;
                                    }
                                    if (tp & 0x80000000u) {               // an element's own entry: "the other sorts before you" + lcp
                                        RACY_STORE_U32(&plist[pi], (lo_first ? 0x81000000u : 0x80000000u) | (uint32_t)d);
                                    } else {                              // a pair: the same for both members
                                        tinfo[hi] = (uint16_t)(lo_first ? 0x8000u | (uint32_t)d : 0u);
                                        tinfo[lo] = (uint16_t)(lo_first ? 0u : 0x8000u | (uint32_t)d);
                                    }
                                } else if ((ent >> 24) == 0xFFu && tid % G == 0) {
                                    if (round) {                          // deeper than TIE_G1 + TIE_G2 windows: the third stage
                                        const uint32_t q = VDEEP ? FETCH_ADD_U32(&pcnt[3], 1u) : TIE_VDEEP_CAP;
                                        if (q < TIE_VDEEP_CAP) vdeep[q] = (uint16_t)vj;
                                        else flag[VDEEP ? 0 : 1] = 1;     // (the plain build: the tile goes on to the VDEEP one)
                                    } else {
                                        const uint32_t q = FETCH_ADD_U32(&pcnt[2], 1u);
                                        if (q < TIE_DEEP_CAP) deep[q] = (uint16_t)vj;
                                    }
                                }
                            }
                        }
                        TILE_SYNC();
                    }
                    if (round || pcnt[2] == 0) break;
                }
                // ---- third stage: what is still equal after TIE_G1 + TIE_G2 windows (2,300 bases: an exact duplicate of a gene, a
                // segmental duplication; ONE exact 50-kb duplicate in a 256 Mi text left a pair like that in a third of all tiles,
                // each of which then went to the comparison sort: 43 of 58 ms).  One entry at a time, every thread of the workgroup
                // a window of its own, TILE_NT windows per round trip to the text, until the first difference (or the end of the
                // shorter suffix) is in sight: any depth.
                const uint32_t nv = !VDEEP ? 0u : pcnt[3] < TIE_VDEEP_CAP ? pcnt[3] : TIE_VDEEP_CAP;   // block-uniform (more: flag is set)
                for (uint32_t q = 0; q < nv && flag[0] == 0; ++q) {
                    const uint32_t vj = vdeep[q];
                    const uint32_t pi = vj < np ? vj : TIE_LIST_CAP - 1u - (vj - np);
                    const uint32_t ent = plist[pi], lo = ent & 0xFFFu, hi = (ent >> 12) & 0xFFFu;
                    const uint64_t a = (uint64_t)ssa[lo], b2 = (uint64_t)ssa[hi];
                    const uint64_t maxlen = a < n && b2 < n ? n - (a > b2 ? a : b2) : 0;
                    bool settled = false;
                    for (uint64_t w0 = TIE_G1 + TIE_G2; !settled; w0 += TILE_NT) {
                        PAR(tid) {
                            if (tid == 0) pcnt[4] = ~0u;
                        }
                        TILE_SYNC();
                        PAR(tid) {
                            const uint64_t l = (uint64_t)KCH_ * (1u + w0 + tid);
                            TL(twa, tid, 0) = 0;
                            TL(twb, tid, 0) = 0;
                            bool hit = l >= maxlen;
                            if (!hit) {
                                const uint64_t wa = window64<BITS>(P, a + l), wb = window64<BITS>(P, b2 + l);
                                TL(twa, tid, 0) = wa;
                                TL(twb, tid, 0) = wb;
                                hit = wa != wb;
                            }
                            if (hit) ATOMIC_MIN_U32(&pcnt[4], tid);
                        }
                        TILE_SYNC();
                        const uint32_t first = pcnt[4];                                        // block-uniform
                        if (first != ~0u) {
                            PAR(tid) {
                                if (tid == first) {
                                    const uint64_t l = (uint64_t)KCH_ * (1u + w0 + tid);
                                    const uint64_t wa = TL(twa, tid, 0), wb = TL(twb, tid, 0);
                                    uint64_t d = maxlen;
                                    bool lo_first = a > b2;
                                    if (l < maxlen) {
                                        d = l + (uint32_t)caps_clz64(wa ^ wb) / BITS;
                                        d = d < maxlen ? d : maxlen;
                                        lo_first = wa < wb;
                                    }
                                    if (d >= (vj < np ? (1ull << 32) : (1ull << 24))) flag[0] = 1;       // (an lcp the notes cannot hold)
                                    else if (vj >= np) plist[pi] = (lo_first ? 0x81000000u : 0x80000000u) | (uint32_t)d;
                                    else {                                // a pair: both members point at vlcp[q]
                                        vlcp[q] = (uint32_t)d;
                                        tinfo[hi] = (uint16_t)(lo_first ? 0xFFFFu : 0u);
                                        tinfo[lo] = (uint16_t)(lo_first ? 0u : 0xFFFFu);
                                    }
                                }
                            }
                            settled = true;
                        }
                        TILE_SYNC();
                    }
                }
            }
        }
        TILE_SYNC();
        PHASE_MARK(17);                                        // T: the listed ties
        fast = flag[0] == 0 && flag[1] == 0;                   // (the tie phases were the last to raise them)
        if (fast) {
        PAR_FRESH_SET(tid) {
            UNROLL
            for (uint32_t k = 0; k < TILE_EPT; ++k) {
                const uint32_t e = tid + k * TILE_NT;
                if (!PERM) TL(rl, tid, k) = 0;
                if (e < cnt) {
                    const uint32_t info = TL(rt, tid, k);
                    const uint32_t ties = info >> 28, slot = TL(rd, tid, k), own = (info >> 8) & 0xFFFu;
                    const uint32_t bs = TL(rb, tid, k) & 0xFFFFu;
                    uint32_t more = 0, best = 0;
                    if (ties == 1u) {
                        const uint32_t v = tinfo[slot];
                        if (v & 0x8000u) {
                            more = 1;
                            best = v & 0x7FFFu;
                            if (VDEEP && best == 0x7FFFu) {                // settled in the third stage: its pair's lcp is in vlcp
                                const uint32_t nq = pcnt[3] < TIE_VDEEP_CAP ? pcnt[3] : TIE_VDEEP_CAP;
                                for (uint32_t q = 0; q < nq; ++q) {
                                    const uint32_t vj = vdeep[q];
                                    if (vj < pcnt[0]) { const uint32_t en = plist[vj]; if ((en & 0xFFFu) == slot || ((en >> 12) & 0xFFFu) == slot) best = vlcp[q]; }
                                }
                            }
                            if (TEST_DROP) best = 0;                       // (tests: the note is lost)
                        }
                    } else if (ties >= 2u && ties <= TIE_LIST_MAX) {
                        for (uint32_t q = 0; q < ties; ++q) {
                            const uint32_t r = plist[TIE_LIST_CAP - 1u - (own + q)];
                            if (r & 0x01000000u) { ++more; best = (r & 0xFFFFFFu) > best ? (r & 0xFFFFFFu) : best; }
                        }
                    } else if (ties > TIE_LIST_MAX) {
                        more = bmore[own];                                 // (phase B)
                        best = bbest[own];
                    }
                    const uint32_t d = bs + (((info & 0xFFu) + more) & 0xFFu);
                    EQ_CHK(slot < cnt && d < cnt, 12);
                    if (PERM) {
                        // the lcp with the predecessor, where a tie settled it, stays with the SLOT (the few beyond 15 bits: vslot / vlcp2)
                        uint32_t lc = best;
                        if (VDEEP && lc >= 0x7FFFu) {
                            const uint32_t q = FETCH_ADD_U32(&pcnt[5], 1u);
                            if (q < TIE_VDEEP_CAP) { vslot[q] = (uint16_t)slot; vlcp2[q] = lc; }
                            lc = q < TIE_VDEEP_CAP ? 0x7FFFu : 0u;         // (no room: the emit phase derives it from the text)
                        }
                        tinfo[slot] = (uint16_t)lc;
                        if (d < TILE_E) perm[d] = (uint16_t)slot;          // (always, in a tile that has not failed: d < cnt)
                    } else {
                        TL(rl, tid, k) = best;
                        TL(rk, tid, k) = skey[slot];                       // picked up for the final placement (behind the barrier)
                        TL(rs, tid, k) = ssa[slot];
                        TL(rd, tid, k) = d;
                    }
                }
            }
        }
        TILE_SYNC();
        PHASE_MARK(13);                                        // rank inside the bin
        if (!PERM) {
            PAR_SAME_G(4, tid) {
                UNROLL
                for (uint32_t k = 0; k < TILE_EPT; ++k) {
                    const uint32_t e = tid + k * TILE_NT;
                    if (e < cnt) {
                        const uint32_t d = TL(rd, tid, k);
                        if (!EQ_OK(d < cnt, 13)) continue;
                        skey[d] = TL(rk, tid, k);
                        ssa[d] = TL(rs, tid, k);
                        // = slcp: the lcp with the predecessor, where a tie settled it (the few beyond 15 bits: in vslot / vlcp)
                        uint32_t lc = TL(rl, tid, k);
                        if (VDEEP && lc >= 0x7FFFu) {
                            const uint32_t q = FETCH_ADD_U32(&pcnt[5], 1u);
                            if (q < TIE_VDEEP_CAP) { vslot[q] = (uint16_t)d; vlcp[q] = lc; }
                            lc = q < TIE_VDEEP_CAP ? 0x7FFFu : 0u;         // (no room: the emit phase derives it from the text)
                        }
                        tinfo[d] = (uint16_t)lc;
                    }
                }
            }
            TILE_SYNC();
            PHASE_MARK(14);                                    // place final
        }
        }
    }
#ifdef CAPS_EMUL
    caps_emul_count_tile3(fast);
#endif
    if (!fast) {
        uint32_t* q_ = !VDEEP && redo_deep && flag[0] == 0 ? redo_deep : redo2;        // block-uniform
        PAR(tid) { if (tid == 0) q_[1 + FETCH_ADD_U32(&q_[0], 1u)] = b; }
    } else if (PERM) {
        // sorted order -> HBM through perm (+ LCPs: the tie phases' notes, else from the neighbours' keys, + boundary records)
        PAR(tid) {
            UNROLL
            for (uint32_t k = 0; k < TILE_EPT; ++k) {
                const uint32_t e = tid + k * TILE_NT;
                if (e < cnt) {
                    const uint32_t sl = perm[e];
                    const uint64_t key = skey[sl];
                    const idx_t sa = ssa[sl];
                    uint64_t l = 0;
                    if (with_lcp && e) {
                        uint32_t ov = tinfo[sl];
                        if (VDEEP && ov == 0x7FFFu) ov = eq_big_lcp(vslot, vlcp2, pcnt[5], sl);
                        if (ov) l = ov;
                        else { const uint32_t sp = perm[e - 1]; l = TILE_EMIT_LCP_(skey[sp], ssa[sp], key, sa); }
                    }
                    if (direct) {
                        STREAM_STORE(&fin.sa[start + e], sa);
                        STREAM_STORE(&fin.lcp[start + e], (idx_t)l);
                        if (e == 0) { fin.first_key[g] = key; fin.first_sa[g] = sa; }
                        if (e == cnt - 1) { fin.last_key[g] = key; fin.last_sa[g] = sa; }
                    } else {
                        out_key[start + e] = key;
                        out_sa[start + e] = sa;
                        if (with_lcp) out_lcp[start + e] = (idx_t)l;
                    }
                }
            }
        }
    } else {
        TILE_SORT_EMIT_((!VDEEP || tinfo[e] != 0x7FFFu ? (uint32_t)tinfo[e] : eq_big_lcp(vslot, vlcp, pcnt[5], e)))
    }
    TILE_SYNC();                                                    // the staging arrays are free for the next tile
    if (!VDEEP && fast && flag[1]) {                                // block-uniform: eq_emit_lcp met equal keys without a note
        PAR(tid) { if (tid == 0) redo2[1 + FETCH_ADD_U32(&redo2[0], 1u)] = b; }
    }
    PHASE_MARK(15);                                            // emit (+ LCPs) and the barrier behind it
    qi += K_GRID_DIM;
    } while (PERSIST && qi < n_redo);
}

#undef TILE_SYNC
#define TILE_SYNC() SYNC()
#undef TILE_EMIT_LCP_
#define TILE_EMIT_LCP_(ka, a, kb, b) tile_pair_lcp<BITS, TILE_RUNS>(P, n, ka, a, kb, b, TILE_KEY_SHIFT)

// ---- tile_sort_general_kernel: the tiles tile_sort_kernel could not finish ------------------
// (keys far from uniform inside the tile, or equal keys: repeats), taken from its queue
// (redo[0] = length, redo[1..] = tile ids) by a fixed grid of workgroups, or one per entry (PERSIST).  Comparison based,
// hence independent of the key distribution:
//  1. samplesort in LDS: every 4th element is a sample; the (<= 1023) samples are sorted by
//     rank-merge levels; every element finds its bin among the sorted samples by a branch-free
//     fixed-depth binary search (exact comparator on key ties), a counting sort groups the bins,
//     and each element ranks itself exactly inside its bin (~4 candidates).  ~25 comparison
//     steps per suffix instead of ~78.  Gives up when a bin holds more than TILE_SAMPLE_LIMIT
//     suffixes;
//  2. bottom-up rank-merge levels over the whole tile (reference: merge_sort,
//     src/Suffix_Array.cpp:112-129): every element finds its slot by the same binary search in
//     the sibling run.
// (A second, finer level of interpolation bins for the overflowing bins was tried first: on
// Markov-skewed DNA it rescued < 20 % of the tiles and cost more than it saved.)
constexpr uint32_t TILE_SAMPLE_LIMIT = 64;

// PERSIST = false: one queue entry per workgroup, as in tile_sort_eq_kernel (the caller knows the queue's length)
template <typename idx_t, int BITS, bool FROM_TEXT, bool RUNS, bool PERSIST = true>
GLOBAL_FN LAUNCH_BOUNDS2(TILE_NT, TILE_WAVES_PER_SIMD) tile_sort_general_kernel(KCTX SegDesc sd, const uint32_t* __restrict__ P, uint64_t n,
                                                          uint64_t text_base, uint32_t lcp_mode, uint32_t slot_cap, const uint64_t* in_key,
                                                          const idx_t* in_sa, uint64_t* out_key, idx_t* out_sa, idx_t* out_lcp,
                                                          FinalOut<idx_t> fin, const uint32_t* __restrict__ redo, uint32_t keys_from_text,
                                                          uint64_t* __restrict__ bflag)
{
    // bflag != null: ties are deferred ("Deferred ties" above) -- equal keys are ordered by position, descending (the comparators
    // run as if the text had length 0: text.h), their LCPs are TIE_SENTINEL, and bflag[segment] says that the segment holds some
    const uint64_t n_cmp = bflag ? 0 : n;
    const uint32_t TILE_KEY_SHIFT = 0;
    (void)TILE_KEY_SHIFT;
    SHARED_ARRAY(uint64_t, skey, TILE_E);
    SHARED_ARRAY(idx_t, ssa, TILE_E);
    SHARED_ARRAY(uint64_t, smk, 2 * TILE_NT);       // samples (2x: the fixed-depth search may probe past the end)
    SHARED_ARRAY(idx_t, sms, 2 * TILE_NT);
    SHARED_ARRAY(uint32_t, hist, TILE_NT + 1);      // bin counters: #bins = #samples + 1 <= TILE_NT
    SHARED_ARRAY(uint32_t, flag, 1);
    TL_DECL(uint64_t, rk, TILE_EPT);
    TL_DECL(idx_t, rs, TILE_EPT);
    TL_DECL(uint32_t, rd, TILE_EPT);
    TL_DECL(uint32_t, rb, TILE_EPT);
    TL_DECL(uint64_t, sk1, 1);                      // the thread's sample while the samples are sorted
    TL_DECL(idx_t, ss1, 1);
    TL_DECL(uint32_t, sd1, 1);
    constexpr bool TILE_RUNS = RUNS;
    const uint32_t n_redo = redo[0];
    uint32_t qi = K_BLOCK_IDX;
    if (qi >= n_redo) return;
    do {
    const uint32_t b = redo[1 + qi];
    const uint32_t g = sd.tile_rec[b].g;
    const TileInfo t = tile_info(sd, b);
    const uint64_t start = t.s0 + (uint64_t)t.tl * TILE_E;
    const uint32_t cnt = (uint32_t)(t.s1 - start < TILE_E ? t.s1 - start : TILE_E);
    const bool with_lcp = lcp_mode != 0 && (t.s1 - t.s0) <= TILE_E;
    const bool direct = with_lcp && fin.sa != nullptr;
    // a bucket that outgrew its slot was put together at its place in the output arrays (tile_sort_kernel, the start of a tile): sorted in place
    const bool in_slot = !TILE_OUTGROWN;
    const uint64_t in0 = slot_cap != 0 && in_slot ? (uint64_t)g * slot_cap : start;
    const uint64_t* src_key = tile_src(in_key, out_key, !in_slot);
    const idx_t* src_sa = in_slot ? in_sa : out_sa;
    const uint32_t S = cnt / 4 < TILE_NT - 1 ? cnt / 4 : TILE_NT - 1;      // samples
    PAR(tid) {
        if (tid == 0) flag[0] = 0;
        for (uint32_t i = tid; i <= TILE_NT; i += K_BLOCK_DIM) hist[i] = 0;
        UNROLL
        for (uint32_t k = 0; k < TILE_EPT; ++k) {
            const uint32_t e = tid + k * TILE_NT;
            if (e < cnt) {
                uint64_t key;
                idx_t sa;
                if (FROM_TEXT) {
                    key = window64<BITS>(P, text_base + start + e);
                    sa = (idx_t)(text_base + start + e);
                } else if (keys_from_text) {                      // 32-bit keys in the slots: the 64-bit key is cut from the text
                    sa = src_sa[in0 + e];
                    key = window64<BITS>(P, (uint64_t)sa);
                } else {
                    key = src_key[in0 + e];
                    sa = src_sa[in0 + e];
                }
                TL(rk, tid, k) = key;
                TL(rs, tid, k) = sa;
                skey[e] = key;
                ssa[e] = sa;
            }
        }
    }
    SYNC();
    bool done = false;
    if (S >= 16) {
        // ---- 1. samplesort.  Samples: one per thread, sorted by rank-merge levels.
        const uint32_t stride = cnt / S;
        PAR(tid) {
            if (tid < S) { smk[tid] = skey[tid * stride]; sms[tid] = ssa[tid * stride]; }
        }
        SYNC();
        for (uint32_t R = 1; R < S; R <<= 1) {
            PAR(tid) {
                uint64_t key1[1] = {0};
                idx_t sa1[1] = {0};
                uint32_t lo1[1] = {0}, hi1[1] = {0};
                uint32_t dbase = 0;
                if (tid < S) {
                    key1[0] = smk[tid];
                    sa1[0] = sms[tid];
                    const uint32_t run = tid / R;
                    uint32_t sib = (run ^ 1u) * R;
                    if (sib > S) sib = S;
                    lo1[0] = sib;
                    hi1[0] = sib + R < S ? sib + R : S;
                    dbase = (run & ~1u) * R + (tid - run * R) - sib;
                }
                multi_lower_bound<idx_t, BITS, 1, RUNS>(P, n_cmp, smk, sms, key1, sa1, lo1, hi1, 2 * R);
                TL(sk1, tid, 0) = key1[0];
                TL(ss1, tid, 0) = sa1[0];
                TL(sd1, tid, 0) = dbase + lo1[0];
            }
            SYNC();
            PAR(tid) {
                if (tid < S) { smk[TL(sd1, tid, 0)] = TL(sk1, tid, 0); sms[TL(sd1, tid, 0)] = TL(ss1, tid, 0); }
            }
            SYNC();
        }
        // bin(x) = #samples < x  (bin j = (sample j-1, sample j]); counting sort by bin
        const uint32_t top = pow2_above(S);
        PAR(tid) {
            UNROLL
            for (uint32_t gg = 0; gg < TILE_EPT; gg += LOCK_K) {
                uint64_t key[LOCK_K];
                idx_t sa[LOCK_K];
                uint32_t lo[LOCK_K], hi[LOCK_K];
                UNROLL
                for (uint32_t k = 0; k < LOCK_K; ++k) {
                    const uint32_t e = tid + (gg + k) * TILE_NT;
                    key[k] = TL(rk, tid, gg + k);
                    sa[k] = TL(rs, tid, gg + k);
                    lo[k] = 0;
                    hi[k] = e < cnt ? S : 0u;
                }
                multi_lower_bound<idx_t, BITS, LOCK_K, RUNS>(P, n_cmp, smk, sms, key, sa, lo, hi, top);
                UNROLL
                for (uint32_t k = 0; k < LOCK_K; ++k) {
                    const uint32_t e = tid + (gg + k) * TILE_NT;
                    if (e < cnt) {
                        const uint32_t r = FETCH_ADD_U32(&hist[lo[k]], 1u);
                        if (r >= TILE_SAMPLE_LIMIT) flag[0] = 1;
                        TL(rb, tid, gg + k) = lo[k];
                        TL(rd, tid, gg + k) = r;
                    }
                }
            }
        }
        SYNC();
        if (flag[0] == 0) {
            block_exclusive_scan<TILE_NT>(KCTX_PASS hist);        // hist[j] = first slot of bin j, hist[TILE_NT] = cnt
            PAR(tid) {
                UNROLL
                for (uint32_t k = 0; k < TILE_EPT; ++k) {
                    const uint32_t e = tid + k * TILE_NT;
                    if (e < cnt) {
                        const uint32_t slot = hist[TL(rb, tid, k)] + TL(rd, tid, k);
                        skey[slot] = TL(rk, tid, k);
                        ssa[slot] = TL(rs, tid, k);
                        TL(rd, tid, k) = slot;
                    }
                }
            }
            SYNC();
            PAR(tid) {
                UNROLL
                for (uint32_t k = 0; k < TILE_EPT; ++k) {
                    const uint32_t e = tid + k * TILE_NT;
                    if (e < cnt) {
                        const uint32_t bin = TL(rb, tid, k), slot = TL(rd, tid, k);
                        const uint32_t bs = hist[bin], be = hist[bin + 1];
                        const uint64_t key = TL(rk, tid, k);
                        const uint64_t sa = (uint64_t)TL(rs, tid, k);
                        uint32_t less = 0;                        // members of my bin that sort before me
                        for (uint32_t j = bs; j < be; ++j)
                            if (j != slot && suffix_less<BITS, RUNS>(P, n_cmp, skey[j], (uint64_t)ssa[j], key, sa)) ++less;
                        TL(rd, tid, k) = bs + less;
                    }
                }
            }
            SYNC();
            TILE_SORT_PLACE_FINAL
            done = true;
        }
    }
#ifdef CAPS_EMUL
    caps_emul_count_tile2(done);
#endif
    // ---- 2. bottom-up rank-merge levels
    if (!done && S >= 16) {
        PAR(tid) {                                  // the counting sort may have been abandoned half way: restore
            UNROLL
            for (uint32_t k = 0; k < TILE_EPT; ++k) {
                const uint32_t e = tid + k * TILE_NT;
                if (e < cnt) { skey[e] = TL(rk, tid, k); ssa[e] = TL(rs, tid, k); }
            }
        }
        SYNC();
    }
    for (uint32_t R = 1; !done && R < cnt; R <<= 1) {
        PAR(tid) {
            UNROLL
            for (uint32_t gg = 0; gg < TILE_EPT; gg += LOCK_K) {          // LOCK_K searches in lockstep
                uint64_t key[LOCK_K];
                idx_t sa[LOCK_K];
                uint32_t lo[LOCK_K], hi[LOCK_K], dbase[LOCK_K];
                UNROLL
                for (uint32_t k = 0; k < LOCK_K; ++k) {
                    const uint32_t e = tid + (gg + k) * TILE_NT;
                    key[k] = 0;
                    sa[k] = 0;
                    lo[k] = hi[k] = dbase[k] = 0;
                    if (e < cnt) {
                        key[k] = skey[e];
                        sa[k] = ssa[e];
                        const uint32_t run = e / R;
                        uint32_t sib_start = (run ^ 1u) * R;
                        if (sib_start > cnt) sib_start = cnt;
                        lo[k] = sib_start;                               // #sibling elements < (key, sa)
                        hi[k] = sib_start + R < cnt ? sib_start + R : cnt;
                        dbase[k] = (run & ~1u) * R + (e - run * R) - sib_start;
                    }
                }
                multi_lower_bound<idx_t, BITS, LOCK_K, RUNS>(P, n_cmp, skey, ssa, key, sa, lo, hi, 2 * R);
                UNROLL
                for (uint32_t k = 0; k < LOCK_K; ++k) {
                    TL(rk, tid, gg + k) = key[k];
                    TL(rs, tid, gg + k) = sa[k];
                    TL(rd, tid, gg + k) = dbase[k] + lo[k];
                }
            }
        }
        SYNC();
        TILE_SORT_PLACE_FINAL
    }
#undef TILE_EMIT_LCP_
#define TILE_EMIT_LCP_(ka, a, kb, b) deferring_pair_lcp<BITS, TILE_RUNS, idx_t>(P, n, bflag, g, ka, a, kb, b)
    TILE_SORT_EMIT
#undef TILE_EMIT_LCP_
#define TILE_EMIT_LCP_(ka, a, kb, b) tile_pair_lcp<BITS, TILE_RUNS>(P, n, ka, a, kb, b, TILE_KEY_SHIFT)
    SYNC();                                        // before the next queued tile re-uses the LDS
    qi += K_GRID_DIM;
    } while (PERSIST && qi < n_redo);
}
#ifdef CAPS_PAR_SWITCHED
#pragma pop_macro("PAR")
#undef CAPS_PAR_SWITCHED
#endif

// ----------------------------------------------------------------------------------
// a3: LCP-merge of run pairs (reference: merge, src/Suffix_Array.cpp:48-109).
//
// A pass merges, inside every segment, runs (2q, 2q+1) of length R into runs of 2R.
// The output of a pair is cut into tiles of TILE_E outputs.
//
//  merge_partition_kernel  one thread per tile: "merge path" splits of the tile's first
//      and last output diagonal (binary search with the full suffix comparator) -> a
//      48-byte TileDesc {source pieces, destination, flags}.  Segments that are already
//      a single run (len <= R) are marked inactive when skip_finished is set: they stay
//      in the buffer their last pass wrote (parity of passes_for(len)), so skewed
//      partitions cost passes only for their own tiles.
//  merge_pass_kernel       persistent workgroups walk the tiles.  Per tile: the two input
//      pieces (key, sa) are staged in LDS, every element finds its output slot by a
//      binary search in the other piece (rank merge: no divergent serial merge), the
//      merged tile is written back coalesced.  The global loads of the NEXT tile are
//      issued into registers before the rank phase, so HBM latency overlaps the LDS work.
//
// LCPs: keys make the reference's LCP bookkeeping (`m`, `l_x`, cpp:59-79) unnecessary for
// ordering, so intermediate passes move no LCPs at all.  The pass that completes a segment
// (flag FINAL) emits them: LCP_z[k] = lcp(z[k-1], z[k]) from the adjacent keys of the merged
// tile (text only when the keys are equal); the predecessor of the tile's first output is
// the larger of the two elements preceding the pieces; a segment head keeps 0 (cpp:117).
// ----------------------------------------------------------------------------------
struct TileDesc {
    uint64_t srcA, srcB, dst;   // element offsets of the two input pieces and of the output
    uint32_t na, nb;            // piece lengths (na + nb <= TILE_E; 0/0 = inactive tile)
    uint32_t flags;             // TD_*
    uint32_t pad;               // the tile's segment
};
constexpr uint32_t TD_HALO_A = 1, TD_HALO_B = 2, TD_FINAL = 4;

// Number of merge passes a segment of `len` elements takes (runs E, 2E, 4E, ... < len).
HD uint32_t passes_for(uint64_t len)
{
    const uint64_t tiles = (len + TILE_E - 1) / TILE_E;
    return tiles <= 1 ? 0u : (uint32_t)(64 - caps_clz64(tiles - 1));
}

// stable: by key alone, an element of A before an element of B with the same key (deferred ties)
template <typename idx_t, int BITS, bool RUNS = true>
DEV_INLINE uint64_t merge_path_split(const uint32_t* __restrict__ P, uint64_t n, const uint64_t* __restrict__ key,
                                     const idx_t* __restrict__ sa, uint64_t A, uint64_t la, uint64_t B, uint64_t lb, uint64_t d,
                                     bool stable = false)
{
    uint64_t lo = d > lb ? d - lb : 0;
    uint64_t hi = d < la ? d : la;
    while (lo < hi) {                                      // #elements of A among the first d outputs
        const uint64_t mid = (lo + hi) >> 1;
        const uint64_t ia = A + mid, ib = B + (d - 1 - mid);
        const bool a_first = stable ? key[ia] <= key[ib] : suffix_less<BITS, RUNS>(P, n, key[ia], (uint64_t)sa[ia], key[ib], (uint64_t)sa[ib]);
        if (a_first) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

template <typename idx_t, int BITS, bool RUNS>
GLOBAL_FN LAUNCH_BOUNDS(256) merge_partition_kernel(KCTX SegDesc sd, const uint32_t* __restrict__ P, uint64_t n,
                                                    uint64_t R, uint64_t single_la, uint32_t skip_finished, uint32_t need_lcp,
                                                    const uint64_t* __restrict__ key, const idx_t* __restrict__ sa,
                                                    TileDesc* __restrict__ desc, uint64_t* __restrict__ moved, uint32_t defer,
                                                    uint32_t* __restrict__ n_active)
{
    // n_active (zeroed by the caller): counts the descriptors written -- desc[0 .. *n_active) is what merge_pass_kernel walks
    // moved (optional): += elements this pass really merges, one global atomic per workgroup
    // defer: the runs are merged by key alone, stably ("Deferred ties")
    SHARED_ARRAY(uint64_t, acc, 1);
    PAR(tid) { if (tid == 0) acc[0] = 0; }
    SYNC();
    PAR(tid) {
        const uint64_t b = (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (b < sd.tile_off[sd.G]) {
            const TileInfo t = tile_info(sd, (uint32_t)b);
            const uint64_t seglen = t.s1 - t.s0;
            TileDesc d;
            d.srcA = d.srcB = d.dst = 0;
            d.na = d.nb = d.flags = d.pad = 0;
            if (single_la != ~0ull || !skip_finished || seglen > R) {
                const PairInfo pr = pair_info(t, R, single_la);
                const uint64_t tot = pr.la + pr.lb;
                const uint64_t d1 = pr.d0 + TILE_E < tot ? pr.d0 + TILE_E : tot;
                const uint64_t A = pr.a0, B = pr.a0 + pr.la;
                const uint64_t i0 = merge_path_split<idx_t, BITS, RUNS>(P, n, key, sa, A, pr.la, B, pr.lb, pr.d0, defer != 0);
                const uint64_t i1 = d1 < tot ? merge_path_split<idx_t, BITS, RUNS>(P, n, key, sa, A, pr.la, B, pr.lb, d1, defer != 0) : pr.la;
                const uint64_t j0 = pr.d0 - i0, j1 = d1 - i1;
                d.srcA = A + i0;
                d.srcB = B + j0;
                d.dst = pr.a0 + pr.d0;
                d.na = (uint32_t)(i1 - i0);
                d.nb = (uint32_t)(j1 - j0);
                d.flags = (i0 > 0 ? TD_HALO_A : 0u) | (j0 > 0 ? TD_HALO_B : 0u);
                if (need_lcp && (single_la != ~0ull || 2 * R >= seglen)) d.flags |= TD_FINAL;
                d.pad = t.g;                              // the segment (merge_pass_kernel flags it when it defers ties)
            }
            // only the tiles that merge something are listed (in any order: they are independent) -- a pass over a text whose
            // buckets nearly all fit a tile used to walk a million empty descriptors (3 of the 3.7 ms of a pass at 3e9)
            if (d.na + d.nb) desc[FETCH_ADD_U32(n_active, 1u)] = d;
            if (moved && (d.na + d.nb)) ATOMIC_ADD_LDS_U64(&acc[0], (uint64_t)(d.na + d.nb));
        }
    }
    SYNC();
    PAR(tid) { if (tid == 0 && moved && acc[0]) ATOMIC_ADD_U64(moved, acc[0]); }
}

template <typename idx_t, int BITS, bool RUNS>
GLOBAL_FN LAUNCH_BOUNDS2(TILE_NT, TILE_WAVES_PER_SIMD) merge_pass_kernel(KCTX const TileDesc* __restrict__ desc, const uint32_t* __restrict__ n_active,
                                                   const uint32_t* __restrict__ P, uint64_t n,
                                                   const uint64_t* __restrict__ in_key, const idx_t* __restrict__ in_sa,
                                                   uint64_t* __restrict__ out_key, idx_t* __restrict__ out_sa,
                                                   idx_t* __restrict__ out_lcp, uint64_t* __restrict__ bflag)
{
    // bflag != null: deferred ties -- stable merge by key, TIE_SENTINEL for equal neighbours, bflag[segment] = 1 where one was written
    SHARED_ARRAY(uint64_t, skey, TILE_E);
    SHARED_ARRAY(idx_t, ssa, TILE_E);
    TL_DECL(uint64_t, pk, TILE_EPT);      // prefetched (next tile)
    TL_DECL(idx_t, ps, TILE_EPT);
    TL_DECL(uint64_t, rk, TILE_EPT);      // element being ranked
    TL_DECL(idx_t, rs, TILE_EPT);
    TL_DECL(uint32_t, rd, TILE_EPT);

    const uint32_t n_tiles = n_active[0];              // the listed tiles (merge_partition_kernel)
    uint32_t t = K_BLOCK_IDX;
    if (t >= n_tiles) return;
    TileDesc d = desc[t];
    PAR(tid) {
        UNROLL
        for (uint32_t k = 0; k < TILE_EPT; ++k) {
            const uint32_t x = tid + k * TILE_NT;
            if (x < d.na + d.nb) {
                const uint64_t src = x < d.na ? d.srcA + x : d.srcB + (x - d.na);
                TL(pk, tid, k) = in_key[src];
                TL(ps, tid, k) = in_sa[src];
            }
        }
    }
    while (true) {
        const uint32_t na = d.na, cnt = d.na + d.nb;
        const uint32_t top = pow2_above(d.na > d.nb ? d.na : d.nb);      // search depth of this tile
        PAR(tid) {
            UNROLL
            for (uint32_t k = 0; k < TILE_EPT; ++k) {
                const uint32_t x = tid + k * TILE_NT;
                if (x < cnt) { skey[x] = TL(pk, tid, k); ssa[x] = TL(ps, tid, k); }
            }
        }
        SYNC();
        // issue the next tile's loads; they stay in flight during the rank phase
        const uint32_t t_next = t + K_GRID_DIM;
        TileDesc dn = d;
        if (t_next < n_tiles) {
            dn = desc[t_next];
            PAR(tid) {
                UNROLL
                for (uint32_t k = 0; k < TILE_EPT; ++k) {
                    const uint32_t x = tid + k * TILE_NT;
                    if (x < dn.na + dn.nb) {
                        const uint64_t src = x < dn.na ? dn.srcA + x : dn.srcB + (x - dn.na);
                        TL(pk, tid, k) = in_key[src];
                        TL(ps, tid, k) = in_sa[src];
                    }
                }
            }
        }
        PAR(tid) {
            UNROLL
            for (uint32_t g = 0; g < TILE_EPT; g += LOCK_K) {            // LOCK_K searches in lockstep
                uint64_t key[LOCK_K];
                idx_t sa[LOCK_K];
                uint32_t lo[LOCK_K], hi[LOCK_K];
                bool up[LOCK_K];
                UNROLL
                for (uint32_t k = 0; k < LOCK_K; ++k) {
                    const uint32_t x = tid + (g + k) * TILE_NT;
                    key[k] = 0;
                    sa[k] = 0;
                    lo[k] = hi[k] = 0;
                    up[k] = false;
                    if (x < cnt) {
                        key[k] = skey[x];
                        sa[k] = ssa[x];
                        const bool fromA = x < na;
                        lo[k] = fromA ? na : 0u;                         // #elements of the other piece < (key, sa)
                        hi[k] = fromA ? cnt : na;
                        up[k] = !fromA;                                  // (deferred ties: B's elements behind A's equal keys)
                    }
                }
                if (bflag) multi_key_bound<LOCK_K>(skey, key, up, lo, hi, top);
                else multi_lower_bound<idx_t, BITS, LOCK_K, RUNS>(P, n, skey, ssa, key, sa, lo, hi, top);
                UNROLL
                for (uint32_t k = 0; k < LOCK_K; ++k) {
                    // slot = own rank + rank in the other piece = (x - na) + lo for both pieces
                    // (from A: x + (lo - na); from B: (x - na) + lo; unsigned wrap-around is fine)
                    TL(rk, tid, g + k) = key[k];
                    TL(rs, tid, g + k) = sa[k];
                    TL(rd, tid, g + k) = (tid + (g + k) * TILE_NT) - na + lo[k];
                }
            }
        }
        SYNC();
        PAR(tid) {
            UNROLL
            for (uint32_t k = 0; k < TILE_EPT; ++k) {
                const uint32_t x = tid + k * TILE_NT;
                if (x < cnt) {
                    const uint32_t dd = TL(rd, tid, k);
                    skey[dd] = TL(rk, tid, k);
                    ssa[dd] = TL(rs, tid, k);
                }
            }
        }
        SYNC();
        if (d.flags & TD_FINAL) {
            // block-uniform scalar loads: the elements preceding the two pieces
            const bool hA = d.flags & TD_HALO_A, hB = d.flags & TD_HALO_B;
            const uint64_t hAk = hA ? in_key[d.srcA - 1] : 0, hBk = hB ? in_key[d.srcB - 1] : 0;
            const uint64_t hAs = hA ? (uint64_t)in_sa[d.srcA - 1] : 0, hBs = hB ? (uint64_t)in_sa[d.srcB - 1] : 0;
            PAR(tid) {
                UNROLL
                for (uint32_t k = 0; k < TILE_EPT; ++k) {
                    const uint32_t x = tid + k * TILE_NT;
                    if (x < cnt) {
                        const uint64_t key = skey[x];
                        const uint64_t sa = (uint64_t)ssa[x];
                        uint64_t l = 0;
                        if (bflag) {
                            // equal keys anywhere before me = an equal key right before me (the pieces are sorted by key)
                            const bool tie = x ? skey[x - 1] == key : (hA && hAk == key) || (hB && hBk == key);
                            if (tie) { l = (uint64_t)tie_sentinel<idx_t>(); bflag[d.pad] = 1; }
                            else if (x) l = pair_lcp<BITS, false>(P, n, skey[x - 1], (uint64_t)ssa[x - 1], key, sa);
                            else {
                                if (hA) l = pair_lcp<BITS, false>(P, n, hAk, hAs, key, sa);
                                if (hB) { const uint64_t l2 = pair_lcp<BITS, false>(P, n, hBk, hBs, key, sa); l = l2 > l ? l2 : l; }
                            }
                        } else
                        if (x) l = pair_lcp<BITS, RUNS>(P, n, skey[x - 1], (uint64_t)ssa[x - 1], key, sa);
                        else {
                            if (hA) l = pair_lcp<BITS, RUNS>(P, n, hAk, hAs, key, sa);
                            if (hB) { const uint64_t l2 = pair_lcp<BITS, RUNS>(P, n, hBk, hBs, key, sa); l = l2 > l ? l2 : l; }
                        }
                        out_key[d.dst + x] = key;
                        out_sa[d.dst + x] = (idx_t)sa;
                        out_lcp[d.dst + x] = (idx_t)l;
                    }
                }
            }
        } else {
            PAR(tid) {
                UNROLL
                for (uint32_t k = 0; k < TILE_EPT; ++k) {
                    const uint32_t x = tid + k * TILE_NT;
                    if (x < cnt) { out_key[d.dst + x] = skey[x]; out_sa[d.dst + x] = ssa[x]; }
                }
            }
        }
        if (t_next >= n_tiles) break;
        SYNC();
        t = t_next;
        d = dn;
    }
}

// Result of a segmented sort with skip_finished: segment g sits in buffer (passes_for(len_g) & 1)
// (0 = the buffer the tile sort wrote).  finalize_kernel gathers SA and LCP of every segment
// into the caller's arrays and computes the LCP at the head of every segment but the first
// (a11: compute_partition_boundary_lcp, src/Suffix_Array.cpp:431-447); empty segments are
// skipped (the reference runs out of bounds on trailing empty partitions).
template <typename idx_t> struct PingPong {
    const uint64_t* key[2];
    const idx_t* sa[2];
    const idx_t* lcp[2];
};

template <typename idx_t, int BITS>
GLOBAL_FN LAUNCH_BOUNDS(256) finalize_kernel(KCTX SegDesc sd, const uint32_t* __restrict__ P, uint64_t n, PingPong<idx_t> pp,
                                             uint32_t skip_finished, uint32_t uniform_sel, idx_t* __restrict__ dSA,
                                             idx_t* __restrict__ dLCP, FinalOut<idx_t> fin)
{
    const uint32_t b = K_BLOCK_IDX;
    if (b >= sd.tile_off[sd.G]) return;
    const uint32_t g = sd.tile_rec[b].g;
    const TileInfo t = tile_info(sd, b);
    const uint64_t seglen = t.s1 - t.s0;
    // with boundary records (fin): segments completed by the tile sort are already in place
    if (fin.sa != nullptr && seglen <= TILE_E) return;
    const uint64_t start = t.s0 + (uint64_t)t.tl * TILE_E;
    const uint32_t cnt = (uint32_t)(t.s1 - start < TILE_E ? t.s1 - start : TILE_E);
    const uint32_t sel = skip_finished ? (passes_for(seglen) & 1u) : uniform_sel;
    const idx_t* __restrict__ src_sa = pp.sa[sel];
    const idx_t* __restrict__ src_lcp = pp.lcp[sel];
    PAR(tid) {
        for (uint32_t e = tid; e < cnt; e += K_BLOCK_DIM) {
            dSA[start + e] = src_sa[start + e];
            uint64_t l = (uint64_t)src_lcp[start + e];
            if (fin.sa != nullptr) {
                if (e == 0 && t.tl == 0) { fin.first_key[g] = pp.key[sel][start]; fin.first_sa[g] = src_sa[start]; }
                if (start + e == t.s1 - 1) { fin.last_key[g] = pp.key[sel][start + e]; fin.last_sa[g] = src_sa[start + e]; }
            } else if (e == 0 && t.tl == 0 && start > 0) {
                // head of segment g: predecessor = last element of the nearest non-empty segment below
                uint32_t h = g;
                while (h > 0 && sd.seg_start[h] == sd.seg_start[h - 1]) --h;      // skip empty ones
                // seg_start[h] == start; the previous segment [seg_start[h-1], start) is non-empty (start > 0)
                const uint64_t plen = sd.seg_start[h] - sd.seg_start[h - 1];
                const uint32_t psel = skip_finished ? (passes_for(plen) & 1u) : uniform_sel;
                l = pair_lcp<BITS>(P, n, pp.key[psel][start - 1], (uint64_t)pp.sa[psel][start - 1], pp.key[sel][start],
                                   (uint64_t)src_sa[start]);
            }
            dLCP[start + e] = (idx_t)l;
        }
    }
}

// a11 with boundary records: LCP at the head of every non-empty segment but the first =
// lcp(last suffix of the nearest non-empty segment below, first suffix of this one).
template <typename idx_t, int BITS>
GLOBAL_FN LAUNCH_BOUNDS(256) head_lcp_kernel(KCTX const uint32_t* __restrict__ P, uint64_t n, const uint64_t* __restrict__ seg_start,
                                             uint32_t G, FinalOut<idx_t> fin, uint32_t from_text)
{
    // from_text: the boundary records hold 32-bit keys of (possibly) different groups: the head LCPs come from the text
    PAR(tid) {
        const uint64_t g = (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (g < G && g > 0) {
            const uint64_t at = seg_start[g];
            if (seg_start[g + 1] > at && at > 0) {
                uint64_t h = g - 1;
                while (seg_start[h + 1] == seg_start[h]) --h;             // at > 0: a non-empty one exists below
                fin.lcp[at] = from_text ? (idx_t)deep_lcp<BITS>(P, n, (uint64_t)fin.last_sa[h], (uint64_t)fin.first_sa[g], 0)
                                        : (idx_t)pair_lcp<BITS>(P, n, fin.last_key[h], (uint64_t)fin.last_sa[h], fin.first_key[g],
                                                                (uint64_t)fin.first_sa[g]);
            }
        }
    }
}

// Maps a launch-order block id to a logical block id such that the blocks that share
// an XCD (b % 8, MI355X_MICROARCH "Workgroup dispatch") work on a contiguous range of
// logical blocks: consecutive logical blocks -- here the searches over one subarray --
// then hit the same 4 MiB L2.  Speed only; any placement is correct.
DEV_INLINE uint64_t xcd_swizzle(uint64_t b, uint64_t nb)
{
    const uint64_t q = nb / 8, r = nb % 8, x = b % 8, y = b / 8;
    return x * q + (x < r ? x : r) + y;
}

// ---- phase 2 straight from the sorted subarrays (a9 + a10 in one pass) ----------------
// The reference first gathers every partition (p^2 memcpy's, cpp:343-358) and then sorts it.
// On one GPU the bucket split of phase 2 can read the partition THROUGH the partition matrix
// instead: element x of partition j is element  PmT[j][g] + (x - rulerT[j][g])  of sorted
// subarray g, g = the run with rulerT[j][g] <= x < rulerT[j][g+1].  That removes one full
// read + write of (key, sa) -- the collate pass -- from the build.  PmT / rulerT are the
// transposes of Pm / ruler (a partition's runs are then consecutive in memory).
template <typename idx_t> struct RunSrc {
    const idx_t* PmT = nullptr;            // [(p+1) x G1]  PmT[j * G1 + g] = Pm[g][j]
    const idx_t* rulerT = nullptr;         // [p x G1]      rulerT[j * G1 + g] = ruler[g][j]
    const uint64_t* sub_start = nullptr;   // [G1 + 1] element offsets of the sorted subarrays
    const uint32_t* first_run = nullptr;   // [#tiles of the partitions] run holding the tile's first element
    uint32_t G1 = 0;
};

// out[c * rows + r] = in[r * cols + c]; 32 x 32 tiles through LDS, 256 threads.
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(256) transpose_kernel(KCTX const idx_t* __restrict__ in, uint32_t rows, uint32_t cols,
                                              idx_t* __restrict__ out)
{
    SHARED_ARRAY(idx_t, tile, 32 * 33);
    const uint32_t tc = (cols + 31) / 32;
    const uint64_t total = (uint64_t)tc * ((rows + 31) / 32);
    for (uint64_t v = K_BLOCK_IDX; v < total; v += K_GRID_DIM) {
        const uint32_t r0 = (uint32_t)(v / tc) * 32, c0 = (uint32_t)(v % tc) * 32;
        PAR(tid) {
            const uint32_t x = tid & 31, y = tid >> 5;             // 8 rows of 32 per step
            for (uint32_t yy = y; yy < 32; yy += 8)
                if (r0 + yy < rows && c0 + x < cols) tile[yy * 33 + x] = in[(uint64_t)(r0 + yy) * cols + c0 + x];
        }
        SYNC();
        PAR(tid) {
            const uint32_t x = tid & 31, y = tid >> 5;
            for (uint32_t yy = y; yy < 32; yy += 8)
                if (c0 + yy < cols && r0 + x < rows) out[(uint64_t)(c0 + yy) * rows + r0 + x] = tile[x * 33 + yy];
        }
        SYNC();
    }
}

// largest g in [lo, hi] with row[g] <= x   (row[lo] <= x)
template <typename idx_t>
DEV_INLINE uint32_t run_of(const idx_t* row, uint32_t lo, uint32_t hi, uint64_t x)
{
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if ((uint64_t)row[mid] <= x) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// One thread per tile of the partitions: the run that holds the tile's first element.
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(256) runs_plan_kernel(KCTX SegDesc sd, const idx_t* __restrict__ rulerT, uint32_t G1,
                                              uint32_t* __restrict__ first_run)
{
    PAR(tid) {
        const uint64_t b = (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (b < sd.tile_off[sd.G]) {
            const uint32_t j = sd.tile_rec[b].g;
            const TileInfo t = tile_info(sd, (uint32_t)b);
            first_run[b] = run_of<idx_t>(rulerT + (uint64_t)j * G1, 0u, G1 - 1, (uint64_t)t.tl * TILE_E);
        }
    }
}

// The runs a tile of partition j spans, staged in LDS: lrow[k] = rulerT[j][ga + k],
// lsrc[k] = (offset of run ga + k in the phase-1 arrays) - lrow[k], so that element x of the
// partition is phase-1 element lsrc[k] + x.  ns = #runs (<= TILE_E to be staged).
#define RUNS_TILE_SETUP                                                                                         \
    const uint32_t run_a = FROM_RUNS ? rsrc.first_run[b] : 0u;                                                  \
    const uint32_t run_b = !FROM_RUNS ? 0u : (start + cnt >= t.s1) ? rsrc.G1 - 1 : rsrc.first_run[b + 1];       \
    const uint32_t run_ns = run_b - run_a + 1;                                                                  \
    const bool runs_staged = run_ns <= TILE_E;                                                                  \
    const idx_t* run_rowR = rsrc.rulerT + (uint64_t)g * rsrc.G1;                                                \
    const idx_t* run_rowA = rsrc.PmT + (uint64_t)g * rsrc.G1;                                                   \
    const uint64_t run_x0 = start - t.s0;                                                                       \
    (void)run_a; (void)run_b; (void)run_ns; (void)runs_staged; (void)run_rowR; (void)run_rowA; (void)run_x0;

#define RUNS_STAGE(tid)                                                                                         \
    if (runs_staged)                                                                                            \
        for (uint32_t k = tid; k < run_ns; k += K_BLOCK_DIM) {                                                  \
            const idx_t r = run_rowR[run_a + k];                                                                \
            lrow[k] = r;                                                                                        \
            lsrc[k] = rsrc.sub_start[run_a + k] + (uint64_t)run_rowA[run_a + k] - (uint64_t)r;                  \
        }

template <typename idx_t>
DEV_INLINE uint64_t run_source(const RunSrc<idx_t>& rsrc, bool staged, const idx_t* lrow, const uint64_t* lsrc, uint32_t ns,
                               const idx_t* rowR, const idx_t* rowA, uint32_t ga, uint32_t gb, uint64_t x)
{
    if (staged) return lsrc[run_of<idx_t>(lrow, 0u, ns - 1, x)] + x;
    const uint32_t r = run_of<idx_t>(rowR, ga, gb, x);
    return rsrc.sub_start[r] + (uint64_t)rowA[r] + (x - (uint64_t)rowR[r]);
}

constexpr int SRC_ARRAYS = 0, SRC_TEXT = 1, SRC_RUNS = 2;      // where a bucket split reads its elements

// ----------------------------------------------------------------------------------
// Bucketing inside a sort (a4/a10): before the tile sort, every segment longer than a tile
// is split by KEY RANGE into B = ceil(len / BUCKET_TARGET) buckets; bucket(key) is a
// monotone map of the key (linear interpolation between the segment's smallest and largest
// possible key), so the buckets are consecutive slices of the sorted segment and become the
// segments of the tile sort.  On keys that are roughly uniform inside their range (random
// DNA: exactly) every bucket fits one tile and the segment needs NO merge pass -- two
// streaming passes (count, scatter) replace log2(len / TILE_E) merge passes.  Buckets that
// come out larger than a tile (skewed or repetitive text) are finished by the LCP-merge
// passes, which only touch those buckets (skip_finished).
//
//   bucket_plan_kernel     per segment: B, range normalisation (kmin, shift, Bq)
//   bucket_count_kernel    per element: ++count[bucket]      (LDS histogram per tile when B <= BUCKET_LDS)
//   bucket_scatter_kernel  per element: slot = start[bucket] + cursor[bucket]++  (same aggregation)
//   unify_kernel           copies the (few) buckets whose last pass ended in the other ping-pong
//                          buffer back, for consumers that index a segment as one array
// ----------------------------------------------------------------------------------
#ifndef CAPS_BUCKET_EIGHTHS
#define CAPS_BUCKET_EIGHTHS 7
#endif
#ifndef CAPS_SCATTER_SWZ
#define CAPS_SCATTER_SWZ 1
#endif
#ifndef CAPS_COLLATE_SWZ
#define CAPS_COLLATE_SWZ 0
#endif
#ifndef CAPS_TILE_SWZ
#define CAPS_TILE_SWZ 0
#endif
constexpr uint32_t BUCKET_TARGET = (TILE_E * CAPS_BUCKET_EIGHTHS) / 8;   // mean bucket size (headroom for the spread of bucket sizes)
constexpr uint32_t BUCKET_LDS = TILE_BINS_;            // buckets per segment the LDS histogram can hold

// (kmin exclusive unless the first group, kmax inclusive) in 64-bit keys -> [kmin, kmax] in the group's 32-bit keys
DEV_INLINE void key32_range(uint64_t& kmin, uint64_t& kmax, bool kmin_exclusive, uint32_t cs)
{
    const uint64_t lo = kmin_exclusive ? kmin + 1 : kmin;
    if (lo > kmax || (kmin_exclusive && kmin == ~0ull)) { kmin = kmax = 0; return; }      // an empty group
    kmin = key32_of(lo, cs);
    kmax = key32_of(kmax, cs);
}

// range_mode 0: keys span the whole 64-bit range (subarrays of text positions);
// range_mode 1: segment g is partition j = part_off + g of part_total and holds keys in
// [pkey[j-1], pkey[j]] (partitions between pivots; a shard owns a slice of the partitions).
GLOBAL_FN LAUNCH_BOUNDS(256) bucket_plan_kernel(KCTX const uint64_t* __restrict__ seg_start, const uint64_t* __restrict__ seg_end,
                                                uint32_t G, uint32_t range_mode,
                                                const uint64_t* __restrict__ pkey, uint32_t part_off, uint32_t part_total,
                                                uint32_t enable, uint32_t fine, uint32_t sub,
                                                BucketParams* __restrict__ bp, uint64_t* __restrict__ segB,
                                                const uint8_t* __restrict__ gshift)
{
    // range_mode 2: as 1, in the space of the parent's 32-bit keys (key32_of with gshift[parent], text.h)
    // sub > 1: every `sub` consecutive segments are the sub-streams of ONE parent (a group of the direct path, written
    // by level A as one stream per XCD): they share the parent's key range and its buckets.  All of them get the parent's
    // map; the bucket count is credited to the LAST sub-stream only, so that the exclusive scan of segB gives every
    // sub-stream the same first bucket.
    PAR(tid) {
        const uint32_t g = K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (g < G) {
            const uint32_t parent = g / sub, first = parent * sub;
            uint64_t len = 0;
            for (uint32_t x = 0; x < sub && first + x < G; ++x) len += seg_end_of(seg_start, seg_end, first + x) - seg_start[first + x];
            uint64_t kmin = 0, kmax = ~0ull;
            if (range_mode >= 1) {                   // the parent is partition part_off + parent of part_total
                const uint32_t j = part_off + parent;
                if (j > 0) kmin = pkey[j - 1];
                if (j + 1 < part_total) kmax = pkey[j];
                if (range_mode == 2) key32_range(kmin, kmax, j > 0, gshift[j]);
            }
            uint32_t B = 1;
            if (enable && len > TILE_E && kmax > kmin) B = (uint32_t)((len + BUCKET_TARGET - 1) / BUCKET_TARGET);
            // sub-streams never take the scatter's one-bucket shortcut (an identity copy of ONE segment): at least two buckets
            if (sub > 1 && B < 2) B = 2;
            // fine > 1: the map of the equalised split's FINE buckets (bucket_group_kernel): k <= `fine` per bucket slot,
            // as many as the LDS histograms hold.  A whole number per slot, so that the plain split (k consecutive fine
            // buckets per slot) is one of the groupings and the chosen one is never worse; segments with more than
            // BUCKET_LDS / 2 slots keep one fine bucket per slot.
            if (fine > 1 && B > 1 && B <= BUCKET_LDS) {
                const uint32_t k = BUCKET_LDS / B < fine ? BUCKET_LDS / B : fine;
                B *= k;
            }
            const BucketParams q = make_bucket_params(kmin, kmax, B);
            bp[g] = q;
            segB[g] = (g % sub == sub - 1 || g == G - 1) ? B : 0;
        }
    }
}

// Equalised split (the redo path of a bucket split whose slots overflowed: keys far from uniform in the
// segment's range).  The count pass has filled fcount[] for the segment's F FINE buckets (linear map with
// `fine` times the resolution); consecutive fine buckets are grouped greedily into the segment's B bucket
// slots, each group as close to a tile as it gets without exceeding it.  gfirst[slot] = first fine bucket
// of the group (F for unused slots), count[slot] = its exact size: no second count pass.  A fine bucket
// that is larger than a tile by itself is a group of its own (LCP-merge passes finish it, as before); if
// a tile per group needs more slots than the segment has, the capacity is raised to the smallest that fits.
GLOBAL_FN LAUNCH_BOUNDS(256) bucket_group_kernel(KCTX uint32_t G, const uint64_t* __restrict__ segB, const uint64_t* __restrict__ bstart,
                                                 const uint64_t* __restrict__ fsegB, const uint64_t* __restrict__ fstart,
                                                 const uint64_t* __restrict__ fcount, uint64_t* __restrict__ count,
                                                 uint32_t* __restrict__ gfirst)
{
    // One workgroup per segment: the fine counts are staged in LDS with coalesced loads (the greedy walks are serial,
    // and a dependent global load per step made this kernel 5 ms at 8000 segments x 1680 fine buckets), thread 0 walks.
    SHARED_ARRAY(uint64_t, fc, BUCKET_LDS);
    for (uint32_t g = K_BLOCK_IDX; g < G; g += K_GRID_DIM) {
        const uint32_t B = (uint32_t)segB[g], F = (uint32_t)fsegB[g];
        const uint64_t b0 = bstart[g], f0 = fstart[g];
        if (B > BUCKET_LDS || F <= B || F > BUCKET_LDS) {   // no finer map (bucket_plan_kernel): every fine bucket is its own slot
            PAR(tid) {
                for (uint32_t i = tid; i < B; i += K_BLOCK_DIM) { count[b0 + i] = i < F ? fcount[f0 + i] : 0; gfirst[b0 + i] = i; }
            }
            continue;
        }
        PAR(tid) { for (uint32_t f = tid; f < F; f += K_BLOCK_DIM) fc[f] = fcount[f0 + f]; }
        SYNC();
        PAR(tid) {
            if (tid == 0) {
                // capacity of a group: a tile if the slots suffice; otherwise the smallest capacity that fits the segment
                // into its B slots (never worse than the B equal key ranges of the plain split, which is one such grouping)
                uint64_t cap = TILE_E, total = 0;
                for (uint32_t f = 0; f < F; ++f) total += fc[f];
                for (uint64_t lo = TILE_E, hi = total > TILE_E ? total : TILE_E;;) {
                    const uint64_t c_try = lo == TILE_E ? lo : (lo + hi) / 2;     // first probe: a tile
                    uint32_t need = 1;
                    uint64_t run = 0;
                    for (uint32_t f = 0; f < F; ++f) {
                        const uint64_t c = fc[f];
                        if (run > 0 && run + c > c_try) { ++need; run = 0; }
                        run += c;
                    }
                    if (need <= B) { cap = c_try; hi = c_try; if (c_try == TILE_E) break; }
                    else lo = c_try + 1;
                    if (lo >= hi) { cap = hi; break; }
                }
                uint32_t gi = 0;
                uint64_t sum = 0;
                gfirst[b0] = 0;
                for (uint32_t f = 0; f < F; ++f) {
                    const uint64_t c = fc[f];
                    if (sum > 0 && sum + c > cap && gi + 1 < B) {
                        count[b0 + gi] = sum;
                        ++gi;
                        gfirst[b0 + gi] = f;
                        sum = 0;
                    }
                    sum += c;
                }
                count[b0 + gi] = sum;
                for (uint32_t i = gi + 1; i < B; ++i) { count[b0 + i] = 0; gfirst[b0 + i] = F; }
            }
        }
        SYNC();                                          // fc is free for the next segment
    }
}

// Key range of every bucket (inverse of bucket_of, to within rounding: keys just outside are
// clamped into the edge bins of the tile sort, which stays correct), stored as the tile sort's
// bin map over that range.  One thread per bucket.
GLOBAL_FN LAUNCH_BOUNDS(256) bucket_ranges_kernel(KCTX const uint64_t* __restrict__ bstart, uint32_t G,
                                                  const BucketParams* __restrict__ bps, const uint64_t* __restrict__ pkey,
                                                  uint32_t range_mode, uint32_t part_off, uint32_t part_total, uint32_t sub,
                                                  BucketParams* __restrict__ tile_map,
                                                  const BucketParams* __restrict__ fbps, const uint32_t* __restrict__ gfirst,
                                                  const uint8_t* __restrict__ gshift, uint8_t* __restrict__ kshift, uint32_t slot_keys)
{
    // range_mode 2 (32-bit keys): the ranges are in the parent's key32 space; kshift[bucket] = the parent's shift
    // slot_keys != 0 (never with range_mode 2): kshift[bucket] = the shift of the slot keys of the bucket's group (slot_key_shift)
    // gfirst != null (equalised split): bucket slot i is the group of fine buckets [gfirst[i], gfirst[i + 1]) of fbps[g]
    PAR(tid) {
        const uint64_t i = (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (i < bstart[G]) {
            uint32_t a = 0, b = G;                     // parent segment: largest g with bstart[g] <= i
            while (b - a > 1) {
                const uint32_t mid = (a + b) / 2;
                if (bstart[mid] <= i) a = mid; else b = mid;
            }
            const uint32_t g = a;
            const BucketParams bp = bps[g];
            uint64_t kmin = 0, kmax = ~0ull;
            if (range_mode >= 1) {
                const uint32_t j = part_off + g / sub;            // sub-streams of one parent share its buckets (bucket_plan_kernel)
                if (j > 0) kmin = pkey[j - 1];
                if (j + 1 < part_total) kmax = pkey[j];
                if (range_mode == 2) { key32_range(kmin, kmax, j > 0, gshift[j]); kshift[i] = gshift[j]; }
            }
            if (slot_keys && range_mode != 2) kshift[i] = (uint8_t)slot_key_shift(bp.range, bp.B);
            const uint32_t bk = (uint32_t)(i - bstart[g]);
            const double range1 = (double)(kmax - kmin) + 1.0;
            uint64_t l = kmin, h = kmax;
            if (bp.B > 1) {
                uint32_t lo = bk, hi = bk + 1, div = bp.B;
                if (gfirst) {
                    div = fbps[g].B;
                    lo = gfirst[i];
                    hi = bk + 1 < bp.B ? gfirst[i + 1] : div;
                    if (hi <= lo) hi = lo + 1;                         // an unused slot: any range will do
                }
                const double dl = (double)lo / (double)div * range1, dh = (double)hi / (double)div * range1;
                if (lo > 0) l = kmin + (uint64_t)dl;
                if (hi < div) h = kmin + (uint64_t)dh;
                if (h < l) h = l;
            }
            tile_map[i] = make_bucket_params(l, h, TILE_BINS);      // the tile sort's bin map over the bucket's key range
        }
    }
}

// Keys of a tile of consecutive text positions are cut from a copy of the tile's slice of the
// packed text in LDS (one coalesced read of ~1 KiB) instead of three dependent global loads
// per suffix.  TEXT_WIN words cover TILE_E positions + one key + alignment slack for BITS = 8.
constexpr uint32_t TEXT_WIN = TILE_E / 4 + 24;
// cells of the splitter LUT of bucket_scatter_kernel<MAP_SPLIT> (split_lut_kernel)
constexpr uint32_t SPLIT_LUT_BITS = TILE_E >= 4096 ? 12 : TILE_E >= 256 ? 8 : 4;
constexpr uint32_t SPLIT_LUT_CELLS = 1u << SPLIT_LUT_BITS;

// word index (in P) of the first staged word for a tile whose first text position is pos0
template <int BITS> HD uint64_t text_win_base(uint64_t pos0) { return pos0 / TextTraits<BITS>::CPW; }

// MAP: how a key finds its bucket inside its parent segment --
//   MAP_LINEAR   linear interpolation over the segment's key range (bps[g]);
//   MAP_GROUPED  equalised split: fine linear bucket (fbps[g]) -> group table (gfirst) -> bucket slot;
//   MAP_SPLIT    splitter table: bucket = #{splitters < key} among the bps[g].B - 1 sorted keys of the segment's table
//                (split + parent * split_stride, parent = g / in_sub; one table for all when split_stride = 0), staged in
//                LDS and searched branch-free in lockstep for the thread's elements -- through a LUT over the keys' top
//                bits when split_lut is given (level A of the direct path: one table over the whole key range), from
//                scratch otherwise (level B in quantile mode: the knots of the segment's group).  Keys only: all
//                suffixes with one key value land in one bucket, so buckets are consecutive slices of the suffix order.
constexpr int MAP_LINEAR = 0, MAP_GROUPED = 1, MAP_SPLIT = 2;
// Where entry i of a sorted table (<= 4096 entries of 8 bytes) sits in LDS.  A lock-step binary search probes, in step j, the
// entries (2 m + 1) 2^j - 1: a stride of 2^(j + 1) entries -- for j >= 3 every probe of a wave falls into the same LDS banks,
// and the upper steps of the search are serialised up to 32 ways (PMC: 87 % of the LDS cycles of the quantile count pass were
// bank conflicts).  XOR-ing the next two index nibbles into the lowest one (which picks the bank pair inside a 128-byte row)
// spreads those probes over all banks; a bijection inside every aligned block of 4096 entries.
HD uint32_t lds_swz(uint32_t i) { return i ^ ((i >> 4) & 15u) ^ ((i >> 8) & 15u); }
#ifdef CAPS_GA_NO_SWZ              /* measurement: level A's splitter table unswizzled */
#define GA_SWZ(i) (i)
#else
#define GA_SWZ(i) lds_swz(i)
#endif
constexpr uint32_t COUNT_CHUNK = 8;            // tiles per chunk of bucket_count_kernel

// Element i of a scatter's input.  REC: in_key points at records (in_sa is unused).  STREAM: the read-once hint.
template <bool REC, bool STREAM, typename KT, typename idx_t>
DEV_INLINE void load_elem(const KT* __restrict__ in_key, const idx_t* __restrict__ in_sa, uint64_t i, KT& key, idx_t& sa)
{
    if (REC) {
        const KeySaRec* p = reinterpret_cast<const KeySaRec*>(in_key) + i;
        const KeySaRec r = STREAM ? rec_stream_load(p) : *p;
        key = (KT)(((uint64_t)r.key_hi << 32) | r.key_lo);
        sa = (idx_t)r.sa;
    } else {
        key = STREAM ? STREAM_LOAD(&in_key[i]) : in_key[i];
        sa = STREAM ? STREAM_LOAD(&in_sa[i]) : in_sa[i];
    }
}
template <bool REC> DEV_INLINE uint64_t load_elem_key(const uint64_t* __restrict__ in_key, uint64_t i)
{
    if (REC) { const KeySaRec* p = reinterpret_cast<const KeySaRec*>(in_key) + i; return ((uint64_t)p->key_hi << 32) | p->key_lo; }
    return in_key[i];
}

// Persistent workgroups (a tile is little work: launching one workgroup per tile is bound by
// the wave launch rate).
// REC_IN (SRC_ARRAYS): the elements are KeySaRec records (in_key points at them).
template <typename idx_t, int BITS, int SRC, int MAP = MAP_LINEAR, bool REC_IN = false>
GLOBAL_FN LAUNCH_BOUNDS(TILE_NT) bucket_count_kernel(KCTX SegDesc sd, const uint32_t* __restrict__ P, uint64_t n_words,
                                                     uint64_t text_base, const uint64_t* __restrict__ in_key, RunSrc<idx_t> rsrc,
                                                     const BucketParams* __restrict__ bps, const uint64_t* __restrict__ bstart,
                                                     uint64_t* __restrict__ count, const uint64_t* __restrict__ split,
                                                     uint32_t split_stride, uint32_t in_sub, uint16_t* __restrict__ bid)
{
    // bid (MAP_SPLIT, optional): bid[element] = its bucket inside the parent -- the scatter that follows reads it back
    // instead of searching the knots again (10 dependent LDS reads per suffix, as much as everything else it does)
    constexpr bool FROM_TEXT = SRC == SRC_TEXT, FROM_RUNS = SRC == SRC_RUNS;
    SHARED_ARRAY(uint32_t, hist, BUCKET_LDS);
    SHARED_ARRAY(uint64_t, stab, MAP == MAP_SPLIT ? BUCKET_LDS : 1);
    SHARED_ARRAY(uint32_t, twin, FROM_TEXT ? TEXT_WIN : 1);
    SHARED_ARRAY(uint64_t, lsrc, FROM_RUNS ? TILE_E : 1);
    SHARED_ARRAY(idx_t, lrow, FROM_RUNS ? TILE_E : 1);
    // A workgroup takes CHUNKS of consecutive tiles and keeps one LDS histogram across the tiles of a chunk that count into
    // the same buckets (consecutive tiles of a long segment, or of the sub-streams of one parent): the histogram reaches the
    // global counters once per chunk instead of once per tile -- at ~1000 buckets per segment and 4096 elements per tile
    // that flush is one global atomic per 4 elements (genome-like 3e9, quantile mode: 20 of 162 ms were this kernel).
    const uint32_t n_tiles = sd.tile_off[sd.G];
    const uint32_t want = n_tiles / (4u * K_GRID_DIM);
    const uint32_t CH = want < 1u ? 1u : want > COUNT_CHUNK ? COUNT_CHUNK : want;          // short launches keep every workgroup busy
    const uint32_t n_chunks = (n_tiles + CH - 1) / CH;
    for (uint32_t v = K_BLOCK_IDX; v < n_chunks; v += K_GRID_DIM) {
    uint64_t cur_b0 = ~0ull;                           // block-uniform: the buckets the LDS histogram counts for (~0: none)
    uint32_t cur_B = 0;
    const uint32_t b_end = (v + 1) * CH < n_tiles ? (v + 1) * CH : n_tiles;
    for (uint32_t b = v * CH; b < b_end; ++b) {
        const uint32_t g = sd.tile_rec[b].g;
        const TileInfo t = tile_info(sd, b);
        const uint64_t start = t.s0 + (uint64_t)t.tl * TILE_E;
        const uint32_t cnt = (uint32_t)(t.s1 - start < TILE_E ? t.s1 - start : TILE_E);
        const BucketParams bp = bps[g];
        const uint64_t b0 = bstart[g];
        if (bp.B == 1) {                               // the segment is its own bucket
            PAR(tid) { if (tid == 0) ATOMIC_ADD_U64(&count[b0], (uint64_t)cnt); }
            continue;
        }
        const bool lds = bp.B <= BUCKET_LDS;
        const uint64_t w0 = text_win_base<BITS>(text_base + start);
        RUNS_TILE_SETUP
        const uint32_t n_split = MAP == MAP_SPLIT ? bp.B - 1 : 0u;
        const uint64_t* tab = MAP == MAP_SPLIT ? split + (uint64_t)(g / in_sub) * split_stride : nullptr;
        // same buckets as the tile before (and, MAP_SPLIT, the same table: it belongs to the parent that owns the buckets)?
        const bool fresh = !lds || b0 != cur_b0 || bp.B != cur_B;
        PAR(tid) {
            if (fresh) {
                for (uint32_t i = tid; i < cur_B; i += K_BLOCK_DIM)
                    if (hist[i]) ATOMIC_ADD_U64(&count[cur_b0 + i], (uint64_t)hist[i]);
                if (lds) for (uint32_t i = tid; i < bp.B; i += K_BLOCK_DIM) hist[i] = 0;
                if (MAP == MAP_SPLIT && lds) for (uint32_t i = tid; i < n_split; i += K_BLOCK_DIM) stab[lds_swz(i)] = tab[i];
            }
            if (FROM_TEXT)
                for (uint32_t i = tid; i < TEXT_WIN; i += K_BLOCK_DIM) twin[i] = w0 + i < n_words ? P[w0 + i] : 0u;
            if (FROM_RUNS) { RUNS_STAGE(tid) }
        }
        if (fresh) { cur_b0 = lds ? b0 : ~0ull; cur_B = lds ? bp.B : 0u; }
        SYNC();
        const uint32_t top = pow2_above(n_split);
        PAR(tid) {
            uint64_t key[TILE_EPT];
            uint32_t bk[TILE_EPT];
            UNROLL
            for (uint32_t k = 0; k < TILE_EPT; ++k) {
                const uint32_t e = tid + k * TILE_NT;
                key[k] = 0;
                if (e < cnt)
                    key[k] = FROM_TEXT ? window64<BITS>(twin, text_base + start + e - w0 * TextTraits<BITS>::CPW)
                           : FROM_RUNS ? in_key[run_source<idx_t>(rsrc, runs_staged, lrow, lsrc, run_ns, run_rowR, run_rowA,
                                                                  run_a, run_b, run_x0 + e)]
                                       : load_elem_key<REC_IN>(in_key, start + e);
                bk[k] = MAP == MAP_SPLIT ? 0u : bucket_of(bp, key[k]);
            }
            if (MAP == MAP_SPLIT && lds) {                                    // (two loops: one pointer for both tables would
                for (uint32_t st = top >> 1; st >= 1; st >>= 1) {             //  make every probe a flat load)
                    UNROLL
                    for (uint32_t k = 0; k < TILE_EPT; ++k) {
                        const uint32_t idx = bk[k] + st - 1;
                        const uint64_t mk = stab[lds_swz(idx < n_split ? idx : n_split - 1)];
                        if (idx < n_split && mk < key[k]) bk[k] += st;
                    }
                }
            } else if (MAP == MAP_SPLIT) {                                    // more knots than LDS holds: search in HBM
                for (uint32_t st = top >> 1; st >= 1; st >>= 1) {
                    UNROLL
                    for (uint32_t k = 0; k < TILE_EPT; ++k) {
                        const uint32_t idx = bk[k] + st - 1;
                        const uint64_t mk = tab[idx < n_split ? idx : n_split - 1];
                        if (idx < n_split && mk < key[k]) bk[k] += st;
                    }
                }
            }
            UNROLL
            for (uint32_t k = 0; k < TILE_EPT; ++k) {
                const uint32_t e = tid + k * TILE_NT;
                if (e < cnt) {
                    if (lds) FETCH_ADD_U32(&hist[bk[k]], 1u);
                    else ATOMIC_ADD_U64(&count[b0 + bk[k]], 1ull);
                    if (MAP == MAP_SPLIT && bid && lds) bid[start + e] = (uint16_t)bk[k];
                }
            }
        }
        SYNC();                                        // the histogram is complete; the staging arrays are free
    }
    if (cur_B) {
        PAR(tid) {
            for (uint32_t i = tid; i < cur_B; i += K_BLOCK_DIM)
                if (hist[i]) ATOMIC_ADD_U64(&count[cur_b0 + i], (uint64_t)hist[i]);
        }
        SYNC();
    }
    }
}

// sub_start[NB+1] = exclusive scan of count (absolute element offsets of the buckets);
// cursor[NB] starts at 0.  Per tile: LDS histogram of its elements' buckets; one global
// cursor bump per (tile, non-empty bucket); the tile is then re-ordered by bucket in LDS so
// that consecutive lanes write consecutive slots (a bucket receives a run of consecutive
// elements from every tile instead of 64 scattered 8-byte stores per wave instruction).
// KT = uint32_t (SRC_ARRAYS, MAP_LINEAR only): the elements carry 32-bit keys in and out, the map lives in their space.
// SPILL (slots only; the speculative split by knots): what does not fit a slot is not dropped but appended to a stream --
// every (tile, bucket) run that reaches beyond its slot reserves its length there (one global atomic, only then).  An
// entry is (key, index, bucket, position inside the bucket): the cursor's values are positions inside the bucket for ALL its
// elements, so once the sizes are known (the cursors) and scanned, spill_gather_kernel copies the slot's part of every bucket
// that outgrew its slot to the bucket's place in the compact array and spill_place_kernel adds the stream's entries: no
// count pass, and no second scatter for a text whose buckets mostly fit (quantile knots: all but 1-2 %, + the repeats).
template <typename idx_t> struct Spill {
    uint64_t* count = nullptr;     // entries reserved so far (beyond cap: the caller redoes the split with the count pass)
    uint64_t cap = 0;
    uint32_t chunk = 0;            // != 0: tile b of the launch owns entries [b * chunk, (b + 1) * chunk) -- its first runs go there
                                   //   without a trip to `count` (which then starts behind the chunks; unused entries: bucket ~0)
    uint64_t base = 0;             // one past the last slot position: an output offset >= base names entry (offset - base)
    uint64_t* key = nullptr;
    idx_t* sa = nullptr;
    uint32_t* bucket = nullptr;    // bucket of the launch (~0: no entry)
    idx_t* rel = nullptr;          // position inside the bucket
};
constexpr uint32_t SPILL_LONG = 64;                   // runs of this length and more: the workgroup writes (bucket, position) together
constexpr uint32_t SPILL_LONG_CAP = TILE_E / SPILL_LONG;
constexpr uint32_t SPILL_CHUNK = TILE_E / 128 ? TILE_E / 128 : 1;   // a tile of a genome-like text puts 7 elements on the stream, mean

// REC_IN (SRC_ARRAYS, 64-bit keys, 32-bit indices): the elements come in as KeySaRec records (in_key points at them, in_sa is
// unused) -- the stream of level A of the direct path; they leave in two arrays as before.
// ISSUE (REC_IN, MAP_LINEAR: level B of the direct path in linear mode): a tile's memory traffic is ISSUED together.  The plain
// build loads an element, waits for it, classifies it and bumps the histogram before it asks for the next one -- TILE_EPT
// dependent trips to HBM per thread, the first of them behind the trip for the bucket map of the tile's segment and the barrier
// behind the zeroed histogram.  Here all TILE_EPT loads of a thread go out as soon as the tile record gives `start` and `cnt`;
// the bucket map is asked for behind them, the histogram is zeroed and handed over while they travel, and the elements are
// classified from the registers.  The other route (one bucket, or more than the histogram holds) is a block of its own that
// returns: its global atomics are not in the element loop of the route that bumps the LDS histogram.  DRAIN_GLOBAL() stands
// where the compiler's count of outstanding accesses is wrong and costs waits (kernel_lang.h): behind the other route (its exit
// is joined with this route, and the first element would wait for all loads instead of its own), behind the classification
// (a lane that skipped an element still counts its load: the re-ordering would wait for the cursor bumps that are meant to
// travel meanwhile) and in front of the emit (a lane without a bucket to bump still counts the bump: every store pair waited
// for the pair before it).  At none of the three is anything outstanding when the kernel runs, but the unused load of a wave
// that lies beyond the end of a last tile.
// SLOT32 (ISSUE, slots only): the elements leave as 8-byte records (slot_rec above: the key narrowed by the group's shift, the
// index) in ONE array of slots -- out_key, out_sa is unused -- 8 instead of 12 bytes and one run instead of two per (tile,
// bucket).  Classified on the 64-bit key as before; the key is narrowed where the element is placed into LDS, so the staging
// array holds the records (skey; ssa is not used) and the emit is one 8-byte LDS read and one 8-byte store per element.
template <typename idx_t, int BITS, int SRC, int MAP, typename KT = uint64_t, bool SPILL = false, bool REC_IN = false, bool ISSUE = false,
          bool SLOT32 = false>
GLOBAL_FN LAUNCH_BOUNDS(TILE_NT) bucket_scatter_kernel(KCTX SegDesc sd, const uint32_t* __restrict__ P, uint64_t n_words,
                                                       uint64_t text_base, const KT* __restrict__ in_key,
                                                       const idx_t* __restrict__ in_sa, RunSrc<idx_t> rsrc,
                                                       const BucketParams* __restrict__ bps, const uint64_t* __restrict__ bstart,
                                                       const uint64_t* __restrict__ sub_start, uint64_t slot_cap,
                                                       idx_t* __restrict__ cursor,
                                                       KT* __restrict__ out_key, idx_t* __restrict__ out_sa,
                                                       const BucketParams* __restrict__ fbps, const uint32_t* __restrict__ gfirst,
                                                       const uint64_t* __restrict__ split, const uint16_t* __restrict__ split_lut,
                                                       const uint32_t* __restrict__ split_span, uint32_t sub, uint32_t split_stride,
                                                       uint32_t in_sub, const uint16_t* __restrict__ bid, Spill<idx_t> spill)
{
    // sub > 1 (slots only; level A of the direct path): bucket i owns `sub` slots, one per sub-stream; the tiles of a
    // launch are dealt to the sub-streams round-robin by block index, i.e. (observed dispatch order, MI355X_MICROARCH
    // "Workgroup dispatch") one sub-stream per XCD: the short runs that consecutive tiles append to a stream then
    // complete each other's cache lines in ONE L2 instead of leaving partial lines in eight.  Any placement is correct.
    constexpr bool GROUPED = MAP == MAP_GROUPED;
    // gfirst != null: equalised split -- the key's FINE bucket (map fbps[g]) is looked up in the segment's group table
    // (bucket_group_kernel) to get its bucket slot.
    // slot_cap != 0 ("speculative" split, no count pass): bucket i of the launch owns the fixed slot
    // [i * slot_cap, (i + 1) * slot_cap) of the output; cursor[] ends as the exact bucket sizes, and
    // elements that do not fit their slot are dropped -- the caller sees a size > slot_cap and
    // redoes the split with the count pass.  slot_cap == 0: bucket i starts at sub_start[i].
    const bool spec = slot_cap != 0;
    const idx_t NO_SLOT = (idx_t)~(idx_t)0;
#if CAPS_SCATTER_SWZ
    const uint32_t v = sub > 1 ? K_BLOCK_IDX                             // sub-streams: tile -> stream by block index
                               : (uint32_t)xcd_swizzle(K_BLOCK_IDX, K_GRID_DIM);   // tiles of one segment on one XCD: the partial
                                                                         // lines of neighbouring runs meet in its L2
#else
    const uint32_t v = K_BLOCK_IDX;
#endif
    const uint32_t sx = sub > 1 ? K_BLOCK_IDX % sub : 0u;
    if (v >= sd.tile_off[sd.G]) return;
    const uint32_t b = v;
    const uint32_t g = sd.tile_rec[b].g;
    const TileInfo t = tile_info(sd, b);
    const uint64_t start = t.s0 + (uint64_t)t.tl * TILE_E;
    const uint32_t cnt = (uint32_t)(t.s1 - start < TILE_E ? t.s1 - start : TILE_E);
    static_assert(!ISSUE || (REC_IN && MAP == MAP_LINEAR && !SPILL), "loads first: the records of level A under the linear map");
    static_assert(!SLOT32 || (ISSUE && sizeof(KT) == 8 && sizeof(idx_t) == 4), "slot keys: the build that issues its loads first, 32-bit indices");
    TL_DECL(KT, rk, TILE_EPT);
    TL_DECL(idx_t, rs, TILE_EPT);
    if (ISSUE) {
        // No branch around a load: a lane at or beyond cnt reads the tile's last element again and never uses it.  (Under
        // `if (e < cnt)` a wave can skip a load, so the compiler must wait for ALL loads before the first element is used: the
        // count of the loads behind the one it needs is not known.  Unguarded, the waits are for one load each, in turn.)
        if (cnt == 0) return;                                            // (no tile is empty; the index below needs an element)
        PAR(tid) {
            UNROLL
            for (uint32_t k = 0; k < TILE_EPT; ++k) {
                const uint32_t e = tid + k * TILE_NT;
                load_elem<REC_IN, true>(in_key, in_sa, start + (e < cnt ? e : cnt - 1), TL(rk, tid, k), TL(rs, tid, k));
            }
        }
        ISSUE_FENCE();                                                   // ... ahead of the trip for the bucket map
    }
    const BucketParams bp = bps[g];
    const uint64_t b0 = bstart[g];
    const uint32_t ks = SLOT32 ? slot_key_shift(bp.range, bp.B) : 0u;    // block-uniform: a tile belongs to one group
    const bool grouped = GROUPED && bp.B > 1 && bp.B <= BUCKET_LDS;      // GROUPED: a build of its own, the plain scatter is hot
    const BucketParams fbp = GROUPED ? fbps[g] : bp;
    SHARED_ARRAY(uint32_t, hist, TILE_BINS + 1);          // counts -> exclusive prefix inside the tile
    SHARED_ARRAY(idx_t, obase, TILE_BINS);                // global slot of the tile's first element of bucket i, minus its prefix
                                                          // (idx_t: 72 KiB of LDS at 32-bit indices -> two workgroups per CU)
    static_assert(sizeof(KT) == 8 || (SRC == SRC_ARRAYS && MAP == MAP_LINEAR), "32-bit keys: arrays in, linear map");
    static_assert(!REC_IN || (SRC == SRC_ARRAYS && sizeof(KT) == 8 && sizeof(idx_t) == 4), "records: arrays in, 64-bit keys, 32-bit indices");
    SHARED_ARRAY(KT, skey, TILE_E);
    SHARED_ARRAY(idx_t, ssa, SLOT32 ? 1 : TILE_E);
    SHARED_ARRAY(uint16_t, sbk, TILE_E);
    // SPILL: the long runs of the tile that went to the stream (at, cursor value, length, bucket)
    SHARED_ARRAY(uint64_t, lr_at, SPILL ? SPILL_LONG_CAP : 1);
    SHARED_ARRAY(idx_t, lr_old, SPILL ? SPILL_LONG_CAP : 1);
    SHARED_ARRAY(uint32_t, lr_c, SPILL ? SPILL_LONG_CAP : 1);
    SHARED_ARRAY(uint32_t, lr_b, SPILL ? SPILL_LONG_CAP : 1);
    SHARED_ARRAY(uint32_t, nlong, 2);     // [1]: entries of the tile's own chunk taken so far
    static_assert(!SPILL || (MAP == MAP_SPLIT && sizeof(KT) == 8), "the spill stream: splits by knots, 64-bit keys");
    TL_DECL(uint32_t, rb, TILE_EPT);      // bucket
    TL_DECL(idx_t, rr, TILE_EPT);         // rank inside (tile, bucket) or inside the bucket (idx_t: a bucket of a
                                          // degenerate text can hold more than 2^32 suffixes at 64-bit indices)
    constexpr bool FROM_TEXT = SRC == SRC_TEXT, FROM_RUNS = SRC == SRC_RUNS;
    const bool lds = bp.B > 1 && bp.B <= BUCKET_LDS;
    // FROM_TEXT: the tile's slice of the packed text is staged in the (not yet used) key staging array;
    // FROM_RUNS: the runs the tile spans are staged in the (not yet used) key and index staging arrays
    // (64-bit keys only: the staging arrays are large enough for these guests)
    uint32_t* twin = reinterpret_cast<uint32_t*>(skey);
    uint64_t* lsrc = reinterpret_cast<uint64_t*>(skey);
    idx_t* lrow = ssa;
    uint16_t* gtab = sbk;                                  // fine bucket -> bucket slot of the segment (sbk is written after its last use)
    static_assert(TILE_E >= BUCKET_LDS && BUCKET_LDS <= 65536, "group table fits the bucket-id staging array");
    const uint64_t w0 = text_win_base<BITS>(text_base + start);
    // MAP_SPLIT: the splitter table sits in the key staging array too, behind the text window
    uint64_t* stab = reinterpret_cast<uint64_t*>(skey) + TILE_E / 4;
    uint16_t* slut = reinterpret_cast<uint16_t*>(ssa);    // ... and its LUT in the index staging array
    static_assert(TEXT_WIN * sizeof(uint32_t) <= (TILE_E / 4) * sizeof(uint64_t) && TILE_E / 4 + BUCKET_LDS <= TILE_E,
                  "text window + splitter table fit the key staging array");
    static_assert((SPLIT_LUT_CELLS + 1) * sizeof(uint16_t) <= TILE_E * sizeof(idx_t), "splitter LUT fits the index staging array");
    const uint32_t n_split = MAP == MAP_SPLIT && bp.B > 1 ? bp.B - 1 : 0u;
    const uint64_t* tab = MAP == MAP_SPLIT ? split + (uint64_t)(g / in_sub) * split_stride : nullptr;
    RUNS_TILE_SETUP
    if (ISSUE) {
        if (!lds) {
            // one bucket, or too many for the LDS histogram: the route at the end of the plain build's classification, whole and on
            // its own here -- its global atomics and its exit stay out of the control flow of the route below
            PAR(tid) {
                UNROLL
                for (uint32_t k = 0; k < TILE_EPT; ++k) {
                    const uint32_t e = tid + k * TILE_NT;
                    if (e < cnt) {
                        const uint64_t bi = (b0 + (bp.B == 1 ? 0u : bucket_of(bp, (uint64_t)TL(rk, tid, k)))) * (spec ? sub : 1u) + sx;
                        const uint64_t off = bp.B == 1 ? (start - t.s0) + e : (uint64_t)caps_fetch_add(&cursor[bi], (idx_t)1);
                        if (!spec || off < slot_cap) {
                            const uint64_t dst = (spec ? bi * slot_cap : sub_start[bi]) + off;
                            if (SLOT32) out_key[dst] = (KT)slot_rec((uint64_t)TL(rk, tid, k), ks, (uint32_t)TL(rs, tid, k));
                            else {
                                out_key[dst] = TL(rk, tid, k);
                                out_sa[dst] = TL(rs, tid, k);
                            }
                        }
                    }
                }
                if (spec && bp.B == 1 && tid == 0) caps_fetch_add(&cursor[b0 * sub + sx], (idx_t)cnt);
            }
            DRAIN_GLOBAL();              // (the compiler joins this route's exit with the route below: nothing of it pending there)
            return;
        }
        PAR(tid) {
            for (uint32_t i = tid; i <= TILE_BINS; i += K_BLOCK_DIM) hist[i] = 0;
        }
        // only LDS is handed over here (the zeroed histogram): a barrier of LDS scope, the loads above stay in flight across it
        SYNC_LDS();
        PAR(tid) {
            UNROLL
            for (uint32_t k = 0; k < TILE_EPT; ++k) {
                const uint32_t e = tid + k * TILE_NT;
                if (e < cnt) {
                    const uint32_t bk = bucket_of(bp, (uint64_t)TL(rk, tid, k));
                    TL(rb, tid, k) = bk;
                    TL(rr, tid, k) = FETCH_ADD_U32(&hist[bk], 1u);
                }
            }
        }
        DRAIN_GLOBAL();                  // every load has been waited for where it was used (or is a wave's unused one): said for all lanes
    } else {
    if (lds || FROM_TEXT || FROM_RUNS) {
        PAR(tid) {
            if (lds) for (uint32_t i = tid; i <= TILE_BINS; i += K_BLOCK_DIM) hist[i] = 0;
            if (SPILL && tid < 2) nlong[tid] = 0;
            if (MAP == MAP_SPLIT && lds && !bid) {
                for (uint32_t i = tid; i < n_split; i += K_BLOCK_DIM) stab[lds_swz(i)] = tab[i];
                if (split_lut) for (uint32_t i = tid; i <= SPLIT_LUT_CELLS; i += K_BLOCK_DIM) slut[i] = split_lut[i];
            }
            if (grouped)                                   // slot i owns the fine buckets [gfirst[i], gfirst[i + 1]) (F for unused slots)
                for (uint32_t i = tid; i < bp.B; i += K_BLOCK_DIM) {
                    const uint32_t f0 = gfirst[b0 + i], f1 = i + 1 < bp.B ? gfirst[b0 + i + 1] : fbp.B;
                    for (uint32_t f = f0; f < f1 && f < fbp.B; ++f) gtab[f] = (uint16_t)i;
                }
            if (FROM_TEXT)
                for (uint32_t i = tid; i < TEXT_WIN; i += K_BLOCK_DIM) twin[i] = w0 + i < n_words ? P[w0 + i] : 0u;
            if (FROM_RUNS) { RUNS_STAGE(tid) }
        }
        SYNC();
    }
    if (MAP == MAP_SPLIT && lds && bid) {
        // the count pass has left every element's bucket (bucket_count_kernel): no table, no search
        PAR(tid) {
            UNROLL
            for (uint32_t k = 0; k < TILE_EPT; ++k) {
                const uint32_t e = tid + k * TILE_NT;
                if (e < cnt) {
                    const uint32_t bk = bid[start + e];
                    load_elem<REC_IN, false>(in_key, in_sa, start + e, TL(rk, tid, k), TL(rs, tid, k));
                    TL(rb, tid, k) = bk;
                    TL(rr, tid, k) = FETCH_ADD_U32(&hist[bk], 1u);
                }
            }
        }
    } else if (MAP == MAP_SPLIT && lds) {
        // keys first, then the TILE_EPT table searches of a thread in lockstep (independent LDS reads in flight together)
        // depth of the search: the candidates per LUT cell (block-uniform), or all of the table without a LUT
        const uint32_t top = pow2_above(split_lut ? split_span[0] : n_split);
        TL_DECL(uint32_t, rh, TILE_EPT);
        PAR(tid) {
            UNROLL
            for (uint32_t k = 0; k < TILE_EPT; ++k) {
                const uint32_t e = tid + k * TILE_NT;
                const uint64_t src = start + e;
                uint64_t key = 0;
                idx_t sa = 0;
                if (e < cnt) {
                    if (FROM_TEXT) {
                        key = window64<BITS>(twin, text_base + start + e - w0 * TextTraits<BITS>::CPW);
                        sa = (idx_t)(text_base + start + e);
                    } else { KT key_in; load_elem<REC_IN, true>(in_key, in_sa, src, key_in, sa); key = (uint64_t)key_in; }
                }
                const uint32_t cell = (uint32_t)(key >> (64 - SPLIT_LUT_BITS));
                TL(rk, tid, k) = key;
                TL(rs, tid, k) = sa;
                TL(rb, tid, k) = split_lut ? slut[cell] : 0u;
                TL(rh, tid, k) = split_lut ? slut[cell + 1] : n_split;
            }
            for (uint32_t s = top >> 1; s >= 1; s >>= 1) {
                UNROLL
                for (uint32_t k = 0; k < TILE_EPT; ++k) {
                    const uint32_t idx = TL(rb, tid, k) + s - 1;
                    const uint64_t mk = stab[lds_swz(idx < n_split ? idx : n_split - 1)];
                    if (idx < TL(rh, tid, k) && mk < TL(rk, tid, k)) TL(rb, tid, k) += s;
                }
            }
            UNROLL
            for (uint32_t k = 0; k < TILE_EPT; ++k) {
                const uint32_t e = tid + k * TILE_NT;
                if (e < cnt) TL(rr, tid, k) = FETCH_ADD_U32(&hist[TL(rb, tid, k)], 1u);
            }
        }
    } else {
    PAR(tid) {
        UNROLL
        for (uint32_t k = 0; k < TILE_EPT; ++k) {
            const uint32_t e = tid + k * TILE_NT;
            if (e < cnt) {
                const uint64_t src = FROM_RUNS ? run_source<idx_t>(rsrc, runs_staged, lrow, lsrc, run_ns, run_rowR, run_rowA, run_a,
                                                                   run_b, run_x0 + e)
                                               : start + e;
                KT key_in = 0;
                idx_t sa = 0;
                if (FROM_TEXT) sa = (idx_t)(text_base + start + e);
                else load_elem<REC_IN, true>(in_key, in_sa, src, key_in, sa);
                const uint64_t key = FROM_TEXT ? window64<BITS>(twin, text_base + start + e - w0 * TextTraits<BITS>::CPW) : (uint64_t)key_in;
                uint32_t bk = 0;
                idx_t r;
                if (bp.B == 1) r = e;                                        // identity: the segment is its own bucket
                else {
                    if (MAP == MAP_SPLIT) {                                  // too many splitters for the LDS table: search in HBM
                        uint32_t a = 0, z = bp.B - 1;
                        while (a < z) { const uint32_t mid = (a + z) >> 1; if (tab[mid] < key) a = mid + 1; else z = mid; }
                        bk = a;
                    } else {
                        bk = bucket_of(fbp, key);
                        if (grouped) bk = gtab[bk];
                    }
                    r = lds ? FETCH_ADD_U32(&hist[bk], 1u) : caps_fetch_add(&cursor[(b0 + bk) * (spec ? sub : 1u) + sx], (idx_t)1);
                }
                TL(rk, tid, k) = key;
                TL(rs, tid, k) = sa;
                TL(rb, tid, k) = bk;
                TL(rr, tid, k) = r;
            }
        }
    }
    }
    if (!lds) {                                            // one bucket, or too many for the LDS histogram
        PAR(tid) {
            UNROLL
            for (uint32_t k = 0; k < TILE_EPT; ++k) {
                const uint32_t e = tid + k * TILE_NT;
                if (e < cnt) {
                    // one bucket: slot = same offset inside the segment (64-bit: such a segment can be long)
                    const uint64_t off = (bp.B == 1 ? (start - t.s0) : 0) + TL(rr, tid, k);
                    const uint64_t bi = (b0 + TL(rb, tid, k)) * (spec ? sub : 1u) + sx;
                    if (!spec || off < slot_cap) {
                        const uint64_t dst = (spec ? bi * slot_cap : sub_start[bi]) + off;
                        out_key[dst] = TL(rk, tid, k);
                        out_sa[dst] = TL(rs, tid, k);
                    }
                }
            }
            if (spec && bp.B == 1 && tid == 0) caps_fetch_add(&cursor[b0 * sub + sx], (idx_t)cnt);    // the size of a one-bucket segment
        }
        return;
    }
    }
    SYNC();
    // One global cursor bump per (tile, non-empty bucket).  The returning atomics are only ISSUED here; their results are
    // needed for the output addresses alone, so they travel while the tile is scanned and re-ordered in LDS (barriers of
    // LDS scope in between: __syncthreads() would wait for them).
    constexpr uint32_t BPT = (TILE_BINS + TILE_NT - 1) / TILE_NT;          // buckets per thread
    TL_DECL(idx_t, co, BPT);
    TL_DECL(uint32_t, cc, BPT);
    PAR(tid) {
        UNROLL
        for (uint32_t j = 0; j < BPT; ++j) {
            const uint32_t i = tid + j * TILE_NT;
            const uint32_t c = i < bp.B ? hist[i] : 0u;
            TL(cc, tid, j) = c;
            TL(co, tid, j) = 0;
            if (c) TL(co, tid, j) = caps_fetch_add(&cursor[spec ? (b0 + i) * sub + sx : b0 + i], (idx_t)c);
        }
    }
    block_exclusive_scan_bins(KCTX_PASS hist);             // hist[i] = position of bucket i inside the re-ordered tile
    PAR(tid) {
        UNROLL
        for (uint32_t k = 0; k < TILE_EPT; ++k) {
            const uint32_t e = tid + k * TILE_NT;
            if (e < cnt) {
                const uint32_t bk = TL(rb, tid, k);
                const uint32_t q = hist[bk] + (uint32_t)TL(rr, tid, k);
                if (SLOT32) skey[q] = (KT)slot_rec((uint64_t)TL(rk, tid, k), ks, (uint32_t)TL(rs, tid, k));
                else {
                    skey[q] = TL(rk, tid, k);
                    ssa[q] = TL(rs, tid, k);
                }
                sbk[q] = (uint16_t)bk;
            }
        }
        UNROLL
        for (uint32_t j = 0; j < BPT; ++j) {
            const uint32_t i = tid + j * TILE_NT;
            if (i < bp.B) {
                const uint32_t c = TL(cc, tid, j);
                const idx_t old = TL(co, tid, j);
                idx_t ob = 0;
                if (c) {
                    const uint64_t ci = spec ? (b0 + i) * sub + sx : b0 + i;
                    if (!spec) ob = (idx_t)(sub_start[b0 + i] + old);
                    else if ((uint64_t)old + c <= slot_cap) ob = (idx_t)(ci * slot_cap + old);
                    else if (SPILL && spill.count) {
                        // the run reaches beyond the slot: all of it goes to the stream (what sits in the slot stays a prefix
                        // of the bucket: the cursor only grows, so every later run of this bucket comes here too)
                        // (room in the tile's own chunk first: the trip to the global counter would sit on every tile's critical
                        // path -- measured at 3e9 genome-like: 20.8 ms with it against 19.4 for the same scatter without a stream)
                        uint64_t at = ~0ull;
                        if (spill.chunk) {
                            const uint32_t lo = FETCH_ADD_U32(&nlong[1], c);
                            if ((uint64_t)lo + c <= spill.chunk) at = (uint64_t)b * spill.chunk + lo;
                        }
                        if (at == ~0ull) at = FETCH_ADD_U64(spill.count, (uint64_t)c);
                        ob = NO_SLOT;
                        if (at + c <= spill.cap) {
                            ob = (idx_t)(spill.base + at);
                            if (c < SPILL_LONG) {
                                for (uint32_t j = 0; j < c; ++j) { spill.bucket[at + j] = (uint32_t)(b0 + i); spill.rel[at + j] = (idx_t)(old + j); }
                            } else {
                                const uint32_t q = FETCH_ADD_U32(&nlong[0], 1u);      // (< SPILL_LONG_CAP: the runs of a tile add up to TILE_E)
                                lr_at[q] = at;
                                lr_old[q] = old;
                                lr_c[q] = c;
                                lr_b[q] = (uint32_t)(b0 + i);
                            }
                        }
                    } else ob = NO_SLOT;
                }
                obase[i] = ob;
            }
        }
    }
    if (ISSUE) DRAIN_GLOBAL();           // the cursor bumps, once for every thread (see ISSUE at the head of the kernel): a thread
    SYNC_LDS();                          //   that bumped has waited for its own above, the others had none to wait for
    PAR(tid) {
        UNROLL
        for (uint32_t k = 0; k < TILE_EPT; ++k) {
            const uint32_t q = tid + k * TILE_NT;
            if (q < cnt) {
                const uint32_t bk = sbk[q];
                const idx_t ob = obase[bk];
                if (SPILL && ob != NO_SLOT && (uint64_t)ob >= spill.base) {
                    const uint64_t dst = (uint64_t)ob - spill.base + (q - hist[bk]);
                    spill.key[dst] = skey[q];
                    spill.sa[dst] = ssa[q];
                } else if (ob != NO_SLOT) {
                    const uint64_t dst = (uint64_t)ob + (q - hist[bk]);
                    STREAM_STORE2(&out_key[dst], skey[q]);
                    if (!SLOT32) STREAM_STORE2(&out_sa[dst], ssa[q]);
                }
            }
        }
        if (SPILL) {
            const uint32_t nl = nlong[0];
            for (uint32_t r = 0; r < nl && r < SPILL_LONG_CAP; ++r) {
                const uint64_t at = lr_at[r];
                const idx_t old = lr_old[r];
                const uint32_t c = lr_c[r], bb = lr_b[r];
                for (uint32_t j = tid; j < c; j += K_BLOCK_DIM) { spill.bucket[at + j] = bb; spill.rel[at + j] = (idx_t)(old + j); }
            }
        }
    }
}

// After a scatter with a spill stream: bucket b of the launch has seg_start[b + 1] - seg_start[b] elements (its cursor); where
// that is more than the slot holds -- or the bucket sits out the tile sort (skip: the letter-run buckets, sorted later from the
// compact array) -- the slot's part goes to the bucket's place in the compact array.  The tail of the slot's part of a bucket
// that outgrew the slot may be positions of runs that went to the stream (never written): spill_place_kernel, next on the
// stream, overwrites exactly those.
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(256) spill_gather_kernel(KCTX const uint64_t* __restrict__ seg_start, uint32_t NB, uint64_t slot_cap,
                                                 const uint8_t* __restrict__ skip, const uint64_t* __restrict__ slot_key,
                                                 const idx_t* __restrict__ slot_sa, uint64_t* __restrict__ dst_key,
                                                 idx_t* __restrict__ dst_sa)
{
    // a workgroup looks at 256 consecutive buckets at once (one bucket per thread: a walk bucket by bucket was one memory latency
    // per bucket for the 98 % that have nothing to copy -- 0.6 ms at 977,000 buckets), lists the few that do, copies those together
    SHARED_ARRAY(uint32_t, lst, 256);
    SHARED_ARRAY(uint32_t, ln, 1);
    for (uint64_t base = (uint64_t)K_BLOCK_IDX * 256u; base < NB; base += (uint64_t)K_GRID_DIM * 256u) {
        PAR(tid) { if (tid == 0) ln[0] = 0; }
        SYNC();
        PAR(tid) {
            const uint64_t b = base + tid;
            if (b < NB) {
                const uint64_t len = seg_start[b + 1] - seg_start[b];
                if (len > slot_cap || (len && skip && skip[b])) lst[FETCH_ADD_U32(&ln[0], 1u)] = (uint32_t)b;
            }
        }
        SYNC();
        const uint32_t m = ln[0];                                           // block-uniform
        for (uint32_t q = 0; q < m; ++q) {
            const uint32_t b = lst[q];
            const uint64_t s0 = seg_start[b], len = seg_start[b + 1] - s0;
            const uint64_t cnt = len < slot_cap ? len : slot_cap;
            PAR(tid) {
                for (uint64_t i = tid; i < cnt; i += K_BLOCK_DIM) {
                    dst_key[s0 + i] = slot_key[(uint64_t)b * slot_cap + i];
                    dst_sa[s0 + i] = slot_sa[(uint64_t)b * slot_cap + i];
                }
            }
        }
        SYNC();
    }
}

template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(256) spill_place_kernel(KCTX Spill<idx_t> sp, uint64_t cnt, const uint64_t* __restrict__ seg_start,
                                                uint64_t* __restrict__ dst_key, idx_t* __restrict__ dst_sa)
{
    PAR(tid) {
        for (uint64_t i = (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid; i < cnt; i += (uint64_t)K_GRID_DIM * K_BLOCK_DIM) {
            const uint32_t b = sp.bucket[i];
            if (b == ~0u) continue;
            const uint64_t d = seg_start[b] + (uint64_t)sp.rel[i];
            dst_key[d] = sp.key[i];
            dst_sa[d] = sp.sa[i];
        }
    }
}

// ---- level A of the direct path: the text -> groups, in tiles of GA_E consecutive positions -------------------------
// A dedicated kernel rather than bucket_scatter_kernel<SRC_TEXT, MAP_SPLIT> (kept: it is the same computation on
// TILE_E positions and serves as its cross-check): with ~1000 groups, a 4096-element tile spends as much on its groups
// (histogram, one cursor bump each, scan) as on its elements, and appends runs of 4 elements.  Here a workgroup takes
// GA_E = 4 x TILE_E positions.  Nothing but the tile's slice of the packed text is staged: a key is cut from it when the
// element is classified and again when it is written, so the per-element state between the two is ONE register
// (group << 14 | position in the re-ordered tile), and the re-ordered tile goes out in TILE_E-element chunks through a
// 16 KB permutation buffer -- 60 KB of LDS at 2-bit codes, two workgroups per CU.
//   cursor[sx * K1 + g]  elements of group g appended so far to sub-stream sx (= block index % sub, see
//                        bucket_scatter_kernel); ends as the stream's size -- larger than slot_cap = the stream overflowed,
//                        its surplus was dropped and the caller must not use the result
//   stream (g, sx) owns [(g * sub + sx) * slot_cap, +slot_cap) of out_key / out_sa
#ifndef CAPS_GA_TILES
#define CAPS_GA_TILES 4
#endif
constexpr uint32_t GA_TILES = CAPS_GA_TILES;
constexpr uint32_t GA_E = GA_TILES * TILE_E;
constexpr uint32_t GA_EPT = GA_E / TILE_NT;
static_assert(GA_E <= (1u << 14) && BUCKET_LDS <= (1u << 11), "group << 14 | position fits a register");

// KT = uint32_t: the elements leave with 32-bit keys, key32_of(key, gshift[group]) (text.h).
// REC_OUT (64-bit keys, 32-bit indices): the elements leave as KeySaRec records, out_key points at them (out_sa is unused);
// stream (g, sx) owns the same region, counted in records.
template <typename idx_t, int BITS, typename KT = uint64_t, bool REC_OUT = false>
GLOBAL_FN LAUNCH_BOUNDS2(TILE_NT, TILE_WAVES_PER_SIMD) group_scatter_kernel(KCTX const uint32_t* __restrict__ P, uint64_t n_words,
                                                      uint64_t text_base, uint64_t len, const uint64_t* __restrict__ split, uint32_t K1,
                                                      const uint16_t* __restrict__ split_lut, const uint32_t* __restrict__ split_span,
                                                      uint32_t sub, uint64_t slot_cap, idx_t* __restrict__ cursor,
                                                      KT* __restrict__ out_key, idx_t* __restrict__ out_sa,
                                                      uint32_t tile_first, uint32_t tile_stride,
                                                      const uint64_t* __restrict__ region_start, const uint64_t* __restrict__ region_cap,
                                                      const uint8_t* __restrict__ gshift, uint32_t own_lo, uint32_t own_hi)
{
    // own_lo .. own_hi: only the elements of these groups are kept (counted, re-ordered, written); stream (g, sx) of a kept group
    // owns [((g - own_lo) * sub + sx) * slot_cap, + slot_cap).  A rank of a sharded build scatters the WHOLE text and keeps the
    // groups it owns: no element ever crosses a link (shard.h); one GPU keeps them all (own_lo = 0, own_hi = K1).
    constexpr bool K32 = sizeof(KT) == 4;
    static_assert(!REC_OUT || (!K32 && sizeof(idx_t) == 4), "records: 64-bit keys, 32-bit indices");
    constexpr uint32_t DROP = ~0u;
    SHARED_ARRAY(uint8_t, scs, K32 ? BUCKET_LDS : 1);
    // region_start != null: stream s = g * sub + sx owns [region_start[s], + region_cap[s]) instead of the uniform
    // [s * slot_cap, + slot_cap) -- groups that share a frequent key get the room of all of them (group_caps_kernel).
    // Workgroup b takes tile tile_first + b * tile_stride of [text_base, text_base + len): a rank of a sharded build takes
    // every world-th tile (its share of the text is then a fine-grained interleave, balanced whatever the text's composition
    // does along its length); one GPU: tile_first = 0, tile_stride = 1.
    constexpr uint32_t CPW = TextTraits<BITS>::CPW;
    constexpr uint32_t WIN = GA_E / CPW + 8;                   // words covering GA_E positions + one key
    const idx_t NO_SLOT = (idx_t)~(idx_t)0;
    SHARED_ARRAY(uint32_t, twin, WIN);
    SHARED_ARRAY(uint64_t, stab, BUCKET_LDS);
    SHARED_ARRAY(uint16_t, slut, SPLIT_LUT_CELLS + 2);
    SHARED_ARRAY(uint32_t, hist, TILE_BINS + 1);
    SHARED_ARRAY(idx_t, obase, TILE_BINS);
    SHARED_ARRAY(uint32_t, perm, TILE_E);
    TL_DECL(uint32_t, pk, GA_EPT);
    const uint64_t start = ((uint64_t)tile_first + (uint64_t)K_BLOCK_IDX * tile_stride) * GA_E;
    if (start >= len) return;
    const uint32_t cnt = (uint32_t)(len - start < GA_E ? len - start : GA_E);
    const uint32_t sx = sub > 1 ? K_BLOCK_IDX % sub : 0u;
    const uint32_t n_split = K1 - 1;
    const uint64_t pos0 = text_base + start;
    const uint64_t w0 = pos0 / CPW;
    const uint32_t top = pow2_above(split_span[0]);
    PAR(tid) {
        for (uint32_t i = tid; i <= TILE_BINS; i += K_BLOCK_DIM) hist[i] = 0;
        for (uint32_t i = tid; i < WIN; i += K_BLOCK_DIM) twin[i] = w0 + i < n_words ? P[w0 + i] : 0u;
        for (uint32_t i = tid; i < n_split; i += K_BLOCK_DIM) stab[GA_SWZ(i)] = split[i];
        for (uint32_t i = tid; i <= SPLIT_LUT_CELLS; i += K_BLOCK_DIM) slut[i] = split_lut[i];
        if (K32) for (uint32_t i = tid; i < K1; i += K_BLOCK_DIM) scs[i] = gshift[i];
    }
    SYNC();
    // ---- classify: group = #{splitters < key} (LUT cell -> a few candidates -> branch-free search), rank inside (tile, group)
    // 2-bit codes: a thread classifies GA_EPT CONSECUTIVE positions (when a tile starts on a word boundary: always, GA_E is a
    // multiple of the 16 bases of a word) -- their keys are one 96-bit window of the staged text shifted along, three LDS reads
    // for all of them instead of three each; byte codes keep one position per thread and round
    const bool RUN_OF_POS = BITS == 2 && GA_EPT == CPW && pos0 % CPW == 0;      // block-uniform
    PAR(tid) {
        uint64_t wA = 0;
        uint32_t wC = 0;
        if (RUN_OF_POS) {
            const uint32_t wi = (uint32_t)(pos0 / CPW - w0) + tid;          // the word of my first position
            wA = ((uint64_t)twin[wi] << 32) | twin[wi + 1];
            wC = twin[wi + 2];
        }
        UNROLL
        for (uint32_t kk = 0; kk < GA_EPT; kk += 4) {
            uint64_t key[4];
            uint32_t lo[4], hi[4];
            UNROLL
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t e = RUN_OF_POS ? tid * GA_EPT + kk + j : tid + (kk + j) * TILE_NT;
                const uint32_t sh = BITS * (kk + j);                        // < 32
                key[j] = e >= cnt ? 0 : !RUN_OF_POS ? window64<BITS>(twin, pos0 + e - w0 * CPW)
                                                    : sh ? (wA << sh) | (uint64_t)(wC >> (32u - sh)) : wA;
                const uint32_t cell = (uint32_t)(key[j] >> (64 - SPLIT_LUT_BITS));
                lo[j] = slut[cell];
                hi[j] = slut[cell + 1];
            }
            for (uint32_t st = top >> 1; st >= 1; st >>= 1) {
                UNROLL
                for (uint32_t j = 0; j < 4; ++j) {
                    const uint32_t idx = lo[j] + st - 1;
                    const uint64_t mk = stab[GA_SWZ(idx < n_split ? idx : (n_split ? n_split - 1 : 0))];
                    if (idx < hi[j] && mk < key[j]) lo[j] += st;
                }
            }
            UNROLL
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t e = RUN_OF_POS ? tid * GA_EPT + kk + j : tid + (kk + j) * TILE_NT;
                uint32_t v = DROP;
                if (e < cnt && lo[j] >= own_lo && lo[j] < own_hi) v = (lo[j] << 14) | FETCH_ADD_U32(&hist[lo[j]], 1u);
                TL(pk, tid, kk + j) = v;
            }
        }
    }
    SYNC();
    // ---- one cursor bump per (tile, non-empty group), issued here and consumed after the scan (the returning atomics
    //      travel meanwhile: LDS-scope barriers in between); hist -> first position of every group in the re-ordered tile
    constexpr uint32_t GPT = (TILE_BINS + TILE_NT - 1) / TILE_NT;          // groups per thread
    TL_DECL(idx_t, co, GPT);
    TL_DECL(uint32_t, cc, GPT);
    PAR(tid) {
        UNROLL
        for (uint32_t j = 0; j < GPT; ++j) {
            const uint32_t i = tid + j * TILE_NT;
            const uint32_t c = i < K1 ? hist[i] : 0u;
            TL(cc, tid, j) = c;
            TL(co, tid, j) = 0;
            if (c) TL(co, tid, j) = caps_fetch_add(&cursor[(uint64_t)sx * K1 + i], (idx_t)c);
        }
    }
    block_exclusive_scan_bins(KCTX_PASS hist);
    PAR(tid) {
        UNROLL
        for (uint32_t k = 0; k < GA_EPT; ++k) {
            const uint32_t v = TL(pk, tid, k), g = v >> 14;
            if (v != DROP) TL(pk, tid, k) = (g << 14) | (hist[g] + (v & 0x3FFFu));   // group << 14 | position q in the re-ordered tile
        }
        UNROLL
        for (uint32_t j = 0; j < GPT; ++j) {
            const uint32_t i = tid + j * TILE_NT;
            if (i < K1) {
                const uint32_t c = TL(cc, tid, j);
                idx_t ob = 0;
                if (c) {
                    const idx_t old = TL(co, tid, j);
                    const uint64_t st = (uint64_t)(i - own_lo) * sub + sx;             // (c != 0: a kept group)
                    // (region_start / region_cap point at the first kept stream's entries; the output starts at its region)
                    const uint64_t r0 = region_start ? region_start[st] - region_start[0] : st * slot_cap, rc = region_start ? region_cap[st] : slot_cap;
                    ob = (uint64_t)old + c <= rc ? (idx_t)(r0 + old) : NO_SLOT;
                }
                obase[i] = ob;
            }
        }
    }
    // ---- write the re-ordered tile (its kept elements), TILE_E positions at a time: perm[q] = group << 14 | element
    const uint32_t kept = hist[TILE_BINS];                              // block-uniform (the scan's total)
    for (uint32_t c0 = 0; c0 < kept; c0 += TILE_E) {
        PAR(tid) {
            UNROLL
            for (uint32_t k = 0; k < GA_EPT; ++k) {
                const uint32_t e = RUN_OF_POS ? tid * GA_EPT + k : tid + k * TILE_NT;
                const uint32_t v = TL(pk, tid, k), q = v & 0x3FFFu;
                if (v != DROP && q - c0 < TILE_E) perm[q - c0] = (v & ~0x3FFFu) | e;
            }
        }
        SYNC_LDS();
        PAR(tid) {
            UNROLL
            for (uint32_t k = 0; k < TILE_EPT; ++k) {
                const uint32_t q = c0 + tid + k * TILE_NT;
                if (q < kept) {
                    const uint32_t v = perm[q - c0], g = v >> 14, e = v & 0x3FFFu;
                    const idx_t ob = obase[g];
                    if (ob != NO_SLOT) {
                        const uint64_t dst = (uint64_t)ob + (q - hist[g]);
                        const uint64_t key = window64<BITS>(twin, pos0 + e - w0 * CPW);
                        if (REC_OUT) {
                            store_rec(out_key, dst, key, (idx_t)(pos0 + e));
                        } else {
                            STREAM_STORE2(&out_key[dst], K32 ? (KT)key32_of(key, scs[g]) : (KT)key);
                            STREAM_STORE2(&out_sa[dst], (idx_t)(pos0 + e));
                        }
                    }
                }
            }
        }
        SYNC_LDS();                                  // the chunk's stores need not land before the next chunk is staged
    }
}

// Report of a rank's level A for the other ranks (sharded direct path): out[0 .. n_streams) = stream sizes,
// out[n_streams] = flag word (pivot-key ties), out[n_streams + 1] = size of the largest stream that outgrew its region (0: none).
// region_cap != null (quantile mode): the room of stream (g, sx) is region_cap[(g - own_lo) * sub + sx] instead of cap (K1 = groups,
// the cursors are stream-major: s = sx * K1 + g; streams of groups outside own_lo .. own_hi are empty).
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(256) stream_report_kernel(KCTX const idx_t* __restrict__ cursor, uint32_t n_streams, uint64_t cap,
                                                  const uint32_t* __restrict__ flag, uint64_t* __restrict__ out,
                                                  const uint64_t* __restrict__ region_cap, uint32_t K1, uint32_t sub, uint32_t own_lo,
                                                  uint32_t own_hi)
{
    PAR(tid) {
        const uint32_t s = K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (s < n_streams) {
            const uint64_t z = (uint64_t)cursor[s];
            out[s] = z;
            uint64_t room = cap;
            if (region_cap) {
                const uint32_t g = s % K1, sx = s / K1;
                room = g >= own_lo && g < own_hi ? region_cap[(uint64_t)(g - own_lo) * sub + sx] : 0;
            }
            if (z > room) ATOMIC_MAX_U64(&out[n_streams + 1], z);
        }
        if (s == n_streams) out[n_streams] = flag[0];
    }
}

// Bucket sizes of a speculative split: cursor (idx_t) -> count (u64), the input of the scan.
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(256) widen_kernel(KCTX const idx_t* __restrict__ in, uint64_t cnt, uint64_t* __restrict__ out)
{
    PAR(tid) {
        const uint64_t i = (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (i < cnt) out[i] = (uint64_t)in[i];
    }
}

// Moves every bucket whose data ended in ping-pong buffer 1 (odd number of merge passes) back
// into buffer 0, so that a parent segment is one sorted array again.
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(256) unify_kernel(KCTX SegDesc sd, const uint64_t* __restrict__ key1, const idx_t* __restrict__ sa1,
                                          uint64_t* __restrict__ key0, idx_t* __restrict__ sa0)
{
    const uint32_t b = K_BLOCK_IDX;
    if (b >= sd.tile_off[sd.G]) return;
    const TileInfo t = tile_info(sd, b);
    if ((passes_for(t.s1 - t.s0) & 1u) == 0) return;
    const uint64_t start = t.s0 + (uint64_t)t.tl * TILE_E;
    const uint32_t cnt = (uint32_t)(t.s1 - start < TILE_E ? t.s1 - start : TILE_E);
    PAR(tid) {
        for (uint32_t e = tid; e < cnt; e += K_BLOCK_DIM) {
            key0[start + e] = key1[start + e];
            sa0[start + e] = sa1[start + e];
        }
    }
}

// ----------------------------------------------------------------------------------
// a6: samples and pivots (reference: sample_pivots/select_pivots, cpp:187-222).
// Unlike the reference's truncated gap (cpp:191: the top of every subarray is never
// sampled), sample k sits at the CENTRE of the k-th of ppp equal slices of the
// sorted subarray: the rank of a pivot among the samples is then an unbiased estimate of
// its rank among all suffixes, and the first/last partitions are not p*gap/2 oversized
// (samples at slice ends made them ~10x the mean at C2).  The output does not depend on
// the pivots.
// ----------------------------------------------------------------------------------
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(256) sample_kernel(KCTX const uint64_t* __restrict__ seg_start, uint32_t G, uint32_t ppp,
                                           const uint64_t* __restrict__ key, const idx_t* __restrict__ sa,
                                           uint64_t* __restrict__ out_key, idx_t* __restrict__ out_sa)
{
    PAR(tid) {
        const uint64_t t = (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (t < (uint64_t)G * ppp) {
            const uint32_t g = (uint32_t)(t / ppp), k = (uint32_t)(t % ppp);
            const uint64_t s0 = seg_start[g], len = seg_start[g + 1] - s0;
            const uint64_t at = s0 + ((uint64_t)(2 * k + 1) * len) / (2 * (uint64_t)ppp);
            out_key[t] = key[at];
            out_sa[t] = sa[at];
        }
    }
}

template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(256) pick_pivots_kernel(KCTX const uint64_t* __restrict__ skey, const idx_t* __restrict__ ssa, uint64_t m,
                                                uint32_t p, uint64_t* __restrict__ pkey, idx_t* __restrict__ psa)
{
    PAR(tid) {
        const uint64_t j = (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (j + 1 < p) {
            const uint64_t at = ((j + 1) * m) / p;
            pkey[j] = skey[at];
            psa[j] = ssa[at];
        }
    }
}

// ---- direct path (pipeline.h, Builder::run_direct): pivots straight from the text ----------------
// The reference samples its SORTED subarrays (cpp:187-195) because phase 1 has sorted them anyway.  The
// direct path draws the same number of samples (p * ppp) from the text itself: sample t is one position of
// the t-th of m equal strata of [0, n) (jittered by a hash of t, so that a periodic text does not alias with
// the stride).  Strata are disjoint, hence the sampled suffixes are distinct.
DEV_INLINE uint64_t mix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// pos0 = first text position of the sampled range (a shard samples its own slice), len = its length, m <= len
template <typename idx_t, int BITS>
GLOBAL_FN LAUNCH_BOUNDS(256) sample_text_kernel(KCTX const uint32_t* __restrict__ P, uint64_t pos0, uint64_t len, uint64_t m,
                                                uint64_t* __restrict__ out_key, idx_t* __restrict__ out_sa)
{
    PAR(tid) {
        const uint64_t t = (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (t < m) {
            const uint64_t q = len / m, r = len % m;                    // floor(t * len / m) = t * q + floor(t * r / m)
            const uint64_t lo = t * q + (t * r) / m, hi = (t + 1) * q + ((t + 1) * r) / m;
            const uint64_t pos = pos0 + lo + mix64(t) % (hi - lo);      // hi - lo >= q >= 1
            out_key[t] = window64<BITS>(P, pos);
            out_sa[t] = (idx_t)pos;
        }
    }
}

// Groups of PG consecutive partitions: gkey[g] = the pivot key that closes group g (g < K1 - 1), i.e. group g holds
// the keys in (gkey[g-1], gkey[g]].  flag[0] |= 1 when two consecutive pivot KEYS are equal (some key value is so
// frequent -- a long repeat, an N-block -- that splitting by key alone cannot balance the groups: the caller then
// takes the samplesort path, whose exact comparator splits such stretches).
GLOBAL_FN LAUNCH_BOUNDS(256) group_keys_kernel(KCTX const uint64_t* __restrict__ pkey, uint32_t p, uint32_t PG, uint32_t K1,
                                               uint64_t* __restrict__ gkey, uint32_t* __restrict__ flag)
{
    // flag[3] = longest run of pivots with one key (how much of the text a single key value covers, in partitions)
    PAR(tid) {
        const uint32_t j = K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (j + 2 < p && pkey[j] >= pkey[j + 1]) {
            flag[0] = 1;                                                // benign race: every writer stores 1
            if (j == 0 || pkey[j - 1] != pkey[j]) {                     // head of a run
                uint32_t len = 2;
                while (j + len < p - 1 && pkey[j + len] == pkey[j]) ++len;
#ifdef CAPS_EMUL
                if (len > flag[3]) flag[3] = len;
#else
                atomicMax(&flag[3], len);
#endif
            }
        }
        if (j + 1 < K1) gkey[j] = pkey[(uint64_t)(j + 1) * PG - 1];
        if (j + 1 == K1) gkey[j] = ~0ull;                               // (as a knot table of K1 buckets: the last one is open above)
    }
}

// 32-bit keys (text.h key32_of): gshift[g] = bits all keys of group g share = the common bit prefix of its smallest
// possible key (the previous group key + 1) and its largest (its own group key), at most 32.
GLOBAL_FN LAUNCH_BOUNDS(256) group_shift_kernel(KCTX const uint64_t* __restrict__ gkey, uint32_t K1, uint8_t* __restrict__ gshift)
{
    PAR(tid) {
        const uint32_t g = K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (g < K1) {
            const uint64_t lo = g ? gkey[g - 1] + 1 : 0, hi = g + 1 < K1 ? gkey[g] : ~0ull;
            const uint64_t x = lo ^ hi;
            const uint32_t c = x ? (uint32_t)caps_clz64(x) : 32u;
            gshift[g] = (uint8_t)(lo > hi ? 0u : c < 32u ? c : 32u);       // (lo > hi: gkey[g-1] was the largest key; the group is empty)
        }
    }
}

// Splitter search accelerator of level A (bucket_scatter_kernel<MAP_SPLIT>): the top SPLIT_LUT_BITS bits of a key select a
// cell; lut[c] = #{splitters < smallest key of cell c} (lut[cells] = n_split), so a key of cell c belongs to group
// lut[c] + #{splitters in [lut[c], lut[c+1]) that are < key}: a search over lut[c+1] - lut[c] candidates instead of all of
// them -- 0 to 2 on pivots that are roughly uniform in the key range, whatever it takes on skewed ones: span[0] = the largest
// such count, the (block-uniform) depth of the branch-free search.

GLOBAL_FN LAUNCH_BOUNDS(256) split_lut_kernel(KCTX const uint64_t* __restrict__ split, uint32_t n_split, uint16_t* __restrict__ lut,
                                              uint32_t* __restrict__ span)
{
    PAR(tid) {
        const uint32_t c = K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (c <= SPLIT_LUT_CELLS) {
            uint32_t lo = 0, hi = n_split;                               // #{splitters < cell_lo(c)}; cell_lo(cells) = 2^64
            if (c < SPLIT_LUT_CELLS) {
                const uint64_t cell_lo = (uint64_t)c << (64 - SPLIT_LUT_BITS);
                while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (split[mid] < cell_lo) lo = mid + 1; else hi = mid; }
            } else lo = n_split;
            lut[c] = (uint16_t)lo;
            if (c < SPLIT_LUT_CELLS) {
                uint32_t a = lo, z = n_split;                            // lut[c + 1], recomputed (no dependence on another thread)
                if (c + 1 < SPLIT_LUT_CELLS) {
                    const uint64_t next_lo = (uint64_t)(c + 1) << (64 - SPLIT_LUT_BITS);
                    while (a < z) { const uint32_t mid = (a + z) >> 1; if (split[mid] < next_lo) a = mid + 1; else z = mid; }
                } else a = n_split;
#ifdef CAPS_EMUL
                if (a - lo > span[0]) span[0] = a - lo;
#else
                if (a > lo) atomicMax(&span[0], a - lo);
#endif
            }
        }
    }
}

// The groups as segments in fixed-capacity regions: group g = [g * cap, g * cap + size_g) of the level-A output.
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(256) slot_segments_kernel(KCTX const idx_t* __restrict__ sizes, uint32_t K1, uint32_t sub, uint32_t stream_major,
                                                  uint64_t cap, const uint64_t* __restrict__ region_start,
                                                  const uint64_t* __restrict__ region_cap, uint64_t* __restrict__ seg_start,
                                                  uint64_t* __restrict__ seg_end, uint64_t* __restrict__ total)
{
    // segment s = g * sub + x is sub-stream x of group g; its size is sizes[x * K1 + g] (stream_major: group_scatter_kernel's
    // cursors) or sizes[s] (bucket_scatter_kernel's); its region: [s * cap, + cap), or region_start / region_cap when given
    PAR(tid) {
        const uint32_t G = K1 * sub;
        const uint32_t s = K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (s < G) {
            const uint64_t z = (uint64_t)sizes[stream_major ? (uint64_t)(s % sub) * K1 + s / sub : s];
            const uint64_t r0 = region_start ? region_start[s] : (uint64_t)s * cap, rc = region_start ? region_cap[s] : cap;
            seg_start[s] = r0;
            seg_end[s] = r0 + (z < rc ? z : rc);                       // an overflowed stream is reported through total[1]
            ATOMIC_ADD_U64(total, z);
            if (z > rc) ATOMIC_MAX_U64(total + 1, z);
        }
        if (s == G) seg_start[s] = region_start ? region_start[G - 1] + region_cap[G - 1] : (uint64_t)G * cap;
    }
}

// ---- quantile mode of the direct path (skewed key distributions: every real genome) ------------------------
// skew_probe_kernel: the pivots are quantiles (equal numbers of suffixes between consecutive ones); level B's linear
// bucket map over a group's key range assumes they are also equally SPACED inside the group.  flag[0] |= 1 when some
// partition's share of its group's key range is below SKEW_MIN / (partitions in the group): its buckets would overflow.
constexpr double SKEW_MIN = 0.7;          // uniform keys: 1 +- 4 % (sampling noise of ppp = 700 samples per partition)

GLOBAL_FN LAUNCH_BOUNDS(256) skew_probe_kernel(KCTX const uint64_t* __restrict__ pkey, uint32_t p, uint32_t PG, uint32_t K1,
                                               uint32_t* __restrict__ flag)
{
    PAR(tid) {
        const uint32_t j = K_BLOCK_IDX * K_BLOCK_DIM + tid;           // partition j = keys in (pkey[j-1], pkey[j]]
        if (j < p) {
            const uint32_t g = j / PG, j0 = g * PG, j1 = (j0 + PG < p ? j0 + PG : p);      // its group: partitions [j0, j1)
            if (j1 - j0 >= 2) {
                const double glo = j0 ? (double)pkey[j0 - 1] : 0.0, ghi = j1 < p ? (double)pkey[j1 - 1] : 18446744073709551615.0;
                const double lo = j ? (double)pkey[j - 1] : 0.0, hi = j + 1 < p ? (double)pkey[j] : 18446744073709551615.0;
                if (ghi > glo && (hi - lo) * (double)(j1 - j0) < SKEW_MIN * (ghi - glo)) flag[0] = 1;
            }
        }
    }
}

// knots[k] (k < NB - 1) = the sample at quantile (k + 1) / NB of the sorted samples: bucket k holds the keys in
// (knots[k-1], knots[k]]; the groups are runs of KPG consecutive buckets, gkey[g] = knots[(g + 1) * KPG - 1].
// A FREQUENT key K -- the quantile of two or more consecutive knots: a long repeat, an N-block -- gets a bucket of its own:
// the first knot of its run becomes K - 1, so bucket (K - 1, K] = {K} holds nothing else (run_bucket_mark_kernel finds such
// buckets by knots[k - 1] + 1 == knots[k]) and the keys between the previous knot and K have theirs.
GLOBAL_FN LAUNCH_BOUNDS(256) knots_kernel(KCTX const uint64_t* __restrict__ skey, uint64_t m, uint64_t NB, uint32_t KPG, uint32_t K1,
                                          uint64_t* __restrict__ knots, uint64_t* __restrict__ gkey)
{
    PAR(tid) {
        const uint64_t k = (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (k < NB) {
            // the last bucket of the last group ends at the top of the key range
            uint64_t v = k + 1 < NB ? skey[((k + 1) * m) / NB] : ~0ull;
            if (k + 2 < NB) {
                const uint64_t nx = skey[((k + 2) * m) / NB];
                const uint64_t pv = k ? skey[(k * m) / NB] : 0;
                if (nx == v && (k == 0 ? v > 0 : pv + 1 < v)) --v;        // head of a run of equal knots, with room below
            }
            knots[k] = v;
            if ((k + 1) % KPG == 0 && (k + 1) / KPG < K1) gkey[(k + 1) / KPG - 1] = v;
        }
    }
}

// Capacity of the streams of every group in quantile mode.  Every bucket is expected to hold n / NB suffixes -- except
// that all suffixes of a frequent key land in the FIRST of the buckets whose knot is that key (the others, (key, key],
// stay empty).  So group g is expected to hold (KPG - lead + tail) buckets' worth: lead = its leading buckets that repeat
// the previous group's last knot (empty), tail = the buckets of later groups that repeat its own last knot (theirs go to g).
// caps[g * sub + x] = base * (KPG - lead + tail) / KPG + token: the shares add up to base * K1.
GLOBAL_FN LAUNCH_BOUNDS(256) group_caps_kernel(KCTX const uint64_t* __restrict__ knots, uint64_t NB, uint32_t KPG, uint32_t K1,
                                               uint32_t sub, uint64_t base, uint64_t token, uint64_t* __restrict__ caps)
{
    PAR(tid) {
        const uint32_t g = K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (g < K1) {
            const uint64_t k0 = (uint64_t)g * KPG, k1 = k0 + KPG;       // the group's buckets [k0, k1)
            uint64_t lead = 0, tail = 0;
            if (g > 0) while (k0 + lead < k1 && knots[k0 + lead] == knots[k0 - 1]) ++lead;
            if (lead < KPG) while (k1 + tail < NB && knots[k1 + tail] == knots[k1 - 1]) ++tail;
            const uint64_t worth = KPG - lead + tail;
            const uint64_t c = base * worth / KPG + token;              // base < 2^33, worth < 2^22
            for (uint32_t x = 0; x < sub; ++x) caps[(uint64_t)g * sub + x] = c;
        }
    }
}

// Quantile mode's counterpart of bucket_plan_kernel: every parent (group) has exactly KPG buckets; all its `sub`
// sub-streams carry that map, the bucket count is credited to the last one (see bucket_plan_kernel).
GLOBAL_FN LAUNCH_BOUNDS(256) knot_plan_kernel(KCTX uint32_t G, uint32_t sub, uint32_t KPG, BucketParams* __restrict__ bp,
                                              uint64_t* __restrict__ segB)
{
    PAR(tid) {
        const uint32_t g = K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (g < G) {
            BucketParams q = make_bucket_params(0, ~0ull, KPG);     // only B is used by MAP_SPLIT
            bp[g] = q;
            segB[g] = (g % sub == sub - 1 || g == G - 1) ? KPG : 0;
        }
    }
}

// The tile sort's bin map of every bucket in quantile mode: linear over (knots[i-1], knots[i]].
// has_prev: knots[-1] exists (a shard's slice of the knots that does not start at bucket 0): the lower end of bucket 0.
GLOBAL_FN LAUNCH_BOUNDS(256) knot_ranges_kernel(KCTX const uint64_t* __restrict__ knots, uint64_t NB, BucketParams* __restrict__ tile_map,
                                                uint32_t has_prev)
{
    PAR(tid) {
        const uint64_t i = (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (i < NB) {
            const bool below = i > 0 || has_prev != 0;
            const uint64_t lo = below ? knots[(int64_t)i - 1] : 0, hi = knots[i];
            tile_map[i] = make_bucket_params(lo < hi ? lo + (below ? 1 : 0) : hi, hi, TILE_BINS);
        }
    }
}

// ---- letter-run buckets (text.h "letter runs") ------------------------------------------------------------------
// run_bucket_mark_kernel: bucket i of a quantile split is a LETTER-RUN BUCKET when it holds one key only (knots[i - 1] + 1 ==
// knots[i]: knots_kernel gives every frequent key such a bucket), that key is one letter repeated, and it is larger than a
// tile -- all the suffixes deep inside the N-blocks of a genome (the CLI maps N to G, src/main.cpp:61-68).  Such a bucket
// sits out the tile sort and the LCP-merge passes (skip[i] = 1: no tiles) and is listed ({bucket, start, end, key} in
// list[1 + 4 j ..], list[0] = how many) for run_rekey_kernel / run_emit_kernel, which order it by (terminator class,
// what is left of the run, text behind the run) -- no suffix of it is compared with another through the run.
constexpr uint32_t RUN_BUCKET_MAX = 64;        // listed buckets (4 letters at 2 bits per char; any more stay ordinary)
GLOBAL_FN LAUNCH_BOUNDS(256) run_bucket_mark_kernel(KCTX const uint64_t* __restrict__ knots, uint64_t NB, uint32_t has_prev, uint32_t bits,
                                                    const uint64_t* __restrict__ seg_start, uint8_t* __restrict__ skip,
                                                    uint64_t* __restrict__ list)
{
    PAR(tid) {
        const uint64_t i = (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (i < NB) {
            const uint64_t hi = knots[i], len = seg_start[i + 1] - seg_start[i];
            const bool pure = (i > 0 || has_prev != 0) ? knots[(int64_t)i - 1] + 1 == hi : hi == 0;
            const bool letter = bits == 2 ? is_letter_key<2>(hi) : is_letter_key<8>(hi);
            uint8_t s = 0;
            if (pure && letter && len > TILE_E) {
                const uint64_t j = FETCH_ADD_U64(&list[0], 1);
                if (j < RUN_BUCKET_MAX) {
                    list[1 + 4 * j] = i;
                    list[2 + 4 * j] = seg_start[i];
                    list[3 + 4 * j] = seg_start[i + 1];
                    list[4 + 4 * j] = hi;
                    s = 1;
                }
            }
            skip[i] = s;
        }
    }
}

// key[x] = run_key(sa[x]) for the elements [s0, s1) of a letter-run bucket of key K (in place: the bucket's keys are all K).
template <typename idx_t, int BITS>
GLOBAL_FN LAUNCH_BOUNDS(256) run_rekey_kernel(KCTX const uint32_t* __restrict__ P, uint64_t n, uint64_t s0, uint64_t s1, uint64_t K,
                                              uint64_t* __restrict__ key, const idx_t* __restrict__ sa)
{
    PAR(tid) {
        for (uint64_t x = s0 + (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid; x < s1; x += (uint64_t)K_GRID_DIM * K_BLOCK_DIM)
            key[x] = run_key<(int)sizeof(idx_t), BITS>(P, n, (uint64_t)sa[x], K);
    }
}

// The sorted letter-run bucket [s0, s1) (run keys + positions) -> SA and LCP.  LCPs from the run keys (text.h run_pair_lcp);
// the bucket's head and the head of what follows it in the suffix array (at `total`: the end of the array) are compared with
// their neighbours in dSA through the text -- the segment records of a bucket that sat out the sort hold nothing.
template <typename idx_t, int BITS>
GLOBAL_FN LAUNCH_BOUNDS(256) run_emit_kernel(KCTX const uint32_t* __restrict__ P, uint64_t n, uint64_t s0, uint64_t s1, uint64_t total,
                                             const uint64_t* __restrict__ key, const idx_t* __restrict__ sa,
                                             idx_t* __restrict__ dSA, idx_t* __restrict__ dLCP)
{
    PAR(tid) {
        for (uint64_t x = s0 + (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid; x <= s1; x += (uint64_t)K_GRID_DIM * K_BLOCK_DIM) {
            if (x == s1) {                                       // the element behind the bucket: its LCP with the bucket's last
                if (s1 < total) dLCP[s1] = (idx_t)deep_lcp<BITS, true>(P, n, (uint64_t)sa[s1 - 1], (uint64_t)dSA[s1], 0);
                continue;
            }
            const uint64_t b = (uint64_t)sa[x];
            uint64_t l = 0;
            if (x > s0) l = run_pair_lcp<(int)sizeof(idx_t), BITS>(P, n, key[x - 1], (uint64_t)sa[x - 1], key[x], b);
            else if (s0 > 0) l = deep_lcp<BITS, true>(P, n, (uint64_t)dSA[s0 - 1], b, 0);
            dSA[x] = (idx_t)b;
            dLCP[x] = (idx_t)l;
        }
    }
}

// ----------------------------------------------------------------------------------
// a7/a8: locate every pivot in every sorted segment (reference: upper_bound,
// cpp:252-297, locate_pivots, cpp:225-249).  Pm is the reference's `P` matrix:
// Pm[g*(np+2) .. ] = {0, ub(pivot_0), ..., ub(pivot_{np-1}), len_g}.
// One thread per (segment, pivot); exact comparator (no 65,536-char cutoff, cpp:261).
// ----------------------------------------------------------------------------------
template <typename idx_t, int BITS, bool GALLOP = false>
GLOBAL_FN LAUNCH_BOUNDS(256) locate_kernel(KCTX const uint32_t* __restrict__ P, uint64_t n,
                                           const uint64_t* __restrict__ seg_start, uint32_t G,
                                           const uint64_t* __restrict__ key, const idx_t* __restrict__ sa,
                                           const uint64_t* __restrict__ pkey, const idx_t* __restrict__ psa, uint32_t np,
                                           idx_t* __restrict__ Pm)
{
    const uint32_t bpr = (np + K_BLOCK_DIM - 1) / K_BLOCK_DIM;            // blocks per segment row
    const uint64_t total = (uint64_t)G * bpr;                             // logical blocks (~p^2 / 256: may exceed a dispatch)
    for (uint64_t v = K_BLOCK_IDX; v < total; v += K_GRID_DIM) {
    const uint64_t L = K_GRID_DIM == total ? xcd_swizzle(v, total) : v;
    const uint32_t g = (uint32_t)(L / bpr), jb = (uint32_t)(L % bpr);
    const uint64_t s0 = seg_start[g], len = seg_start[g + 1] - s0;
    PAR(tid) {
        const uint32_t j = jb * K_BLOCK_DIM + tid;
        idx_t* row = Pm + (uint64_t)g * (np + 2);
        if (j < np) {
            const uint64_t pk = pkey[j], ps = (uint64_t)psa[j];
            uint64_t lo = 0, hi = len;                                    // first element > pivot
            // The pivots are quantiles of all suffixes, so pivot j sits near rank (j + 1) * len / (np + 1) of any subarray,
            // whatever the key distribution (binomial spread).  Short subarrays (fewer than 8 elements per pivot: C2 has 4)
            // gallop from that guess to a bracket and bisect there: C2's locate 1.48 -> 0.87 ms.  Long ones keep the plain
            // bisection: its upper levels probe the same few cache lines for all 64 pivots of a wave, while every
            // galloping probe of a wave touches 64 lines (C3, 47 elements per pivot: 4.6 -> 8 ms with the gallop).
            if (GALLOP && len > 64 && len < 8 * (uint64_t)np) {        // a build of its own: the plain one keeps its registers
                const uint64_t g0 = ((uint64_t)(j + 1) * len) / ((uint64_t)np + 1);          // < len
                uint64_t step = 32;
                if (suffix_less<BITS>(P, n, pk, ps, key[s0 + g0], (uint64_t)sa[s0 + g0])) {   // element g0 > pivot: answer <= g0
                    hi = g0;
                    while (hi > 0) {
                        const uint64_t probe = hi > step ? hi - step : 0;
                        if (suffix_less<BITS>(P, n, pk, ps, key[s0 + probe], (uint64_t)sa[s0 + probe])) { hi = probe; step *= 2; }
                        else { lo = probe + 1; break; }
                    }
                } else {                                                                      // answer > g0
                    lo = g0 + 1;
                    while (lo < len) {
                        const uint64_t probe = lo + step - 1 < len ? lo + step - 1 : len - 1;
                        if (!suffix_less<BITS>(P, n, pk, ps, key[s0 + probe], (uint64_t)sa[s0 + probe])) { lo = probe + 1; step *= 2; }
                        else { hi = probe; break; }
                    }
                }
            }
            while (lo < hi) {
                const uint64_t mid = (lo + hi) >> 1;
                if (suffix_less<BITS>(P, n, pk, ps, key[s0 + mid], (uint64_t)sa[s0 + mid])) hi = mid;
                else lo = mid + 1;
            }
            row[j + 1] = (idx_t)lo;
        }
        if (j == 0) { row[0] = 0; row[np + 1] = (idx_t)len; }
    }
    }
}

// ----------------------------------------------------------------------------------
// a9: partition sizes and the "ruler" (reference: partition_sub_subarrays, cpp:300-368).
// Column j of Pm: ruler[g*p + j] = offset of sub-subarray (g, j) inside partition j
// (exclusive scan over g, cpp:340-349), sizes[j] = partition size (cpp:305-316).
// ----------------------------------------------------------------------------------
// Two launches over a (column block) x (row chunk) grid: partial column sums per row chunk,
// then every chunk walks its rows again with the sum of the chunks above it as base.
constexpr uint32_t PART_CHUNKS = 64;

template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(256) partition_partial_kernel(KCTX const idx_t* __restrict__ Pm, uint32_t G, uint32_t p,
                                                      uint64_t* __restrict__ partial)
{
    const uint32_t ncb = (p + K_BLOCK_DIM - 1) / K_BLOCK_DIM;
    const uint32_t cb = K_BLOCK_IDX % ncb, rc = K_BLOCK_IDX / ncb;
    const uint32_t rows = (G + PART_CHUNKS - 1) / PART_CHUNKS;
    const uint32_t g0 = rc * rows, g1 = g0 + rows < G ? g0 + rows : G;
    PAR(tid) {
        const uint32_t j = cb * K_BLOCK_DIM + tid;
        if (j < p) {
            uint64_t run = 0;
            for (uint32_t g = g0; g < g1; ++g) {
                const idx_t* row = Pm + (uint64_t)g * (p + 1);
                run += (uint64_t)(row[j + 1] - row[j]);
            }
            partial[(uint64_t)rc * p + j] = run;
        }
    }
}

template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(256) partition_sizes_kernel(KCTX const idx_t* __restrict__ Pm, uint32_t G, uint32_t p,
                                                    const uint64_t* __restrict__ partial, idx_t* __restrict__ ruler,
                                                    uint64_t* __restrict__ sizes)
{
    const uint32_t ncb = (p + K_BLOCK_DIM - 1) / K_BLOCK_DIM;
    const uint32_t cb = K_BLOCK_IDX % ncb, rc = K_BLOCK_IDX / ncb;
    const uint32_t rows = (G + PART_CHUNKS - 1) / PART_CHUNKS;
    const uint32_t g0 = rc * rows, g1 = g0 + rows < G ? g0 + rows : G;
    PAR(tid) {
        const uint32_t j = cb * K_BLOCK_DIM + tid;
        if (j < p) {
            uint64_t run = 0;
            for (uint32_t c = 0; c < rc; ++c) run += partial[(uint64_t)c * p + j];
            for (uint32_t g = g0; g < g1; ++g) {               // G sorted subarrays (all p, or a shard's slice)
                const idx_t* row = Pm + (uint64_t)g * (p + 1);
                ruler[(uint64_t)g * p + j] = (idx_t)run;
                run += (uint64_t)(row[j + 1] - row[j]);
            }
            if (rc == PART_CHUNKS - 1) sizes[j] = run;
        }
    }
}

// Collate: move every element of sorted subarray g to its slot in its partition
// (reference: the p^2 memcpy's at cpp:343-358).  Element x of subarray g belongs to
// partition j with Pm[g][j] <= x < Pm[g][j+1]; slot = part_start[j] + ruler[g][j] + (x - Pm[g][j]).
// collate_plan_kernel finds the partition of every tile's first element; collate_kernel stages
// the slice of the subarray's Pm row that its tile spans (with the slot bases) in LDS and
// resolves every element there.  Reads are coalesced; writes land in runs of consecutive
// slots.  Only (key, sa) move: phase 2 rebuilds the LCPs (the reference resets run-head LCPs
// here, cpp:356).
constexpr uint32_t COLLATE_ROW = TILE_E + 2;     // row entries a tile can span without empty partitions in between

template <typename idx_t>
DEV_INLINE uint32_t partition_of(const idx_t* __restrict__ row, uint32_t p, uint64_t x)
{
    uint32_t lo = 0, hi = p;                                     // j = #{j' in [1,p] : row[j'] <= x}
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((uint64_t)row[mid + 1] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(256) collate_plan_kernel(KCTX SegDesc sd, uint32_t p, const idx_t* __restrict__ Pm,
                                                 uint32_t* __restrict__ first_part)
{
    PAR(tid) {
        const uint64_t b = (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (b < sd.tile_off[sd.G]) {
            const uint32_t g = sd.tile_rec[b].g;
            const TileInfo t = tile_info(sd, (uint32_t)b);
            first_part[b] = partition_of<idx_t>(Pm + (uint64_t)g * (p + 1), p, (uint64_t)t.tl * TILE_E);
        }
    }
}

template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(TILE_NT) collate_kernel(KCTX SegDesc sd, uint32_t p, const idx_t* __restrict__ Pm,
                                                const idx_t* __restrict__ ruler, const uint64_t* __restrict__ part_start,
                                                const uint32_t* __restrict__ first_part,
                                                const uint64_t* __restrict__ in_key, const idx_t* __restrict__ in_sa,
                                                uint64_t* __restrict__ out_key, idx_t* __restrict__ out_sa)
{
#if CAPS_COLLATE_SWZ
    const uint32_t b = (uint32_t)xcd_swizzle(K_BLOCK_IDX, K_GRID_DIM);
#else
    const uint32_t b = K_BLOCK_IDX;
#endif
    if (b >= sd.tile_off[sd.G]) return;
    const uint32_t g = sd.tile_rec[b].g;
    const TileInfo t = tile_info(sd, b);
    const uint64_t x0 = (uint64_t)t.tl * TILE_E;                  // index of the tile's first element in the subarray
    const uint64_t start = t.s0 + x0;
    const uint32_t cnt = (uint32_t)(t.s1 - start < TILE_E ? t.s1 - start : TILE_E);
    const idx_t* row = Pm + (uint64_t)g * (p + 1);
    const uint32_t j0 = first_part[b];
    // last partition the tile touches: the next tile's first one, or p - 1 at the end of the subarray
    const bool last_tile = start + cnt >= t.s1;
    const uint32_t j1 = last_tile ? p - 1 : first_part[b + 1];
    const uint32_t ns = j1 - j0 + 1;                               // partitions spanned
    SHARED_ARRAY(idx_t, lrow, COLLATE_ROW);                        // row[j0 .. j1 + 1]
    SHARED_ARRAY(uint64_t, lbase, COLLATE_ROW);                    // slot of (partition j, x = 0)
    const bool staged = ns + 1 <= COLLATE_ROW;
    if (staged) {
        PAR(tid) {
            for (uint32_t k = tid; k <= ns; k += K_BLOCK_DIM) {
                const uint32_t j = j0 + k;
                lrow[k] = row[j];
                if (k < ns) lbase[k] = part_start[j] + (uint64_t)ruler[(uint64_t)g * p + j] - (uint64_t)row[j];
            }
        }
        SYNC();
    }
    PAR(tid) {
        UNROLL
        for (uint32_t k = 0; k < TILE_EPT; ++k) {
            const uint32_t e = tid + k * TILE_NT;
            if (e < cnt) {
                const uint64_t x = x0 + e;
                uint64_t dst;
                if (staged) {
                    uint32_t lo = 0, hi = ns - 1;                 // largest k with lrow[k] <= x  (lrow[0] <= x0 <= x)
                    while (lo < hi) {
                        const uint32_t mid = (lo + hi + 1) >> 1;
                        if ((uint64_t)lrow[mid] <= x) lo = mid; else hi = mid - 1;
                    }
                    dst = lbase[lo] + x;
                } else {
                    const uint32_t j = partition_of<idx_t>(row, p, x);
                    dst = part_start[j] + (uint64_t)ruler[(uint64_t)g * p + j] + (x - (uint64_t)row[j]);
                }
                out_key[dst] = in_key[start + e];
                out_sa[dst] = in_sa[start + e];
            }
        }
    }
}

// a2 as a stand-alone entry point: lcp of suffix pairs (a[i], b[i]).
template <typename idx_t, int BITS>
GLOBAL_FN LAUNCH_BOUNDS(256) lcp_pairs_kernel(KCTX const uint32_t* __restrict__ P, uint64_t n, const idx_t* __restrict__ a,
                                              const idx_t* __restrict__ b, uint64_t cnt, idx_t* __restrict__ out)
{
    PAR(tid) {
        const uint64_t i = (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (i < cnt) {
            const uint64_t x = a[i], y = b[i];
            out[i] = (idx_t)(x == y ? n - x : deep_lcp<BITS>(P, n, x, y, 0));
        }
    }
}

// ----------------------------------------------------------------------------------
// Deferred ties, resolved (pipeline.h msd_refine): MSD refinement of the groups of equal keys a sort has left open.
//
// A group = a maximal run of entries of the finished arrays whose LCPs are TIE_SENTINEL, plus the entry before the run (its
// head, whose LCP with ITS predecessor is already right): suffixes that share their first D = KCH chars, at positions
// [pos, pos + len) of SA that are theirs whatever their order turns out to be.  The members are copied to compact work arrays
// (wsa; seg_start / gpos: where a group starts there and in SA), and then, level by level:
//   re-key      key = the KCH chars behind the D known-equal ones: one window of the text per member
//   sort        every group by (key, position descending) -- the ordinary segmented sort, text-free (SortOpts::keys_only)
//   classify    neighbours with different keys are settled: LCP = D + what the two keys share.  Equal keys: still open, unless
//               the upper one's suffix ends inside this window -- then it is a prefix of the lower one (the pad behind the
//               text is the smallest code), sorts first (it has the larger position) and the LCP is its length
//   compact     what is still open (runs of >= 2) moves on, D += KCH
// Groups of at most MSD_FIN_MAX members leave the loop at once: one wave ranks them by direct comparison from depth D on
// (deep_scan: run-table aware, any depth).  The reference settles every one of these pairs by scanning both suffixes from
// their known common prefix (src/Suffix_Array.cpp:69-80 through LCP<8>, include/Suffix_Array.hpp:195-241).
// ----------------------------------------------------------------------------------
#ifndef CAPS_MSD_FIN_MAX
#define CAPS_MSD_FIN_MAX 32
#endif
constexpr uint32_t MSD_FIN_MAX = CAPS_MSD_FIN_MAX;
constexpr uint64_t MSD_TILE_BIT = 1ull << 40;             // tile counts: elements in the low 40 bits, tiles above
constexpr uint64_t MSD_ELEM_MASK = MSD_TILE_BIT - 1;

// tcnt[b] = (elements of tile b) | MSD_TILE_BIT if the tile's segment holds deferred ties, else 0
GLOBAL_FN LAUNCH_BOUNDS(256) msd_tile_counts_kernel(KCTX SegDesc sd, const uint64_t* __restrict__ bflag, uint64_t* __restrict__ tcnt)
{
    PAR(tid) {
        const uint64_t b = (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (b < sd.tile_off[sd.G]) {
            const TileInfo t = tile_info(sd, (uint32_t)b);
            const uint64_t start = t.s0 + (uint64_t)t.tl * TILE_E;
            const uint64_t cnt = t.s1 - start < TILE_E ? t.s1 - start : TILE_E;
            tcnt[b] = bflag[t.g] ? (cnt | MSD_TILE_BIT) : 0;
        }
    }
}

// ftile[j] = the j-th flagged tile (toff = exclusive scan of tcnt)
GLOBAL_FN LAUNCH_BOUNDS(256) msd_tile_list_kernel(KCTX const uint64_t* __restrict__ tcnt, const uint64_t* __restrict__ toff, uint32_t n_tiles,
                                                  uint32_t* __restrict__ ftile)
{
    PAR(tid) {
        const uint64_t b = (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (b < n_tiles && tcnt[b]) ftile[toff[b] >> 40] = (uint32_t)b;
    }
}

// suffix `sa` ends inside (or before) the window of chars [D, D + KCH) of the group's members
template <int BITS> HD bool msd_ending(uint64_t n, uint64_t sa, uint64_t D) { return n - sa <= D + TextTraits<BITS>::KCH; }

// Level 0: the members of the flagged tiles.  flags[toff(tile) + e] = member | head << 32 for entry e of the tile: an entry is
// tied to its predecessor when its LCP is the sentinel.  SA / LCP: the slice the sort wrote (segment offsets).
// (A suffix that ends inside the key is a member like any other -- the merge passes may have left it anywhere in its group;
// it is a prefix of the other members, and the levels / the comparisons below place it first.)
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(256) msd_flags0_kernel(KCTX SegDesc sd, const uint32_t* __restrict__ ftile, const uint64_t* __restrict__ toff,
                                               const idx_t* __restrict__ LCP, uint64_t* __restrict__ flags)
{
    const uint32_t b = ftile[K_BLOCK_IDX];
    const TileInfo t = tile_info(sd, b);
    const uint64_t start = t.s0 + (uint64_t)t.tl * TILE_E;
    const uint32_t cnt = (uint32_t)(t.s1 - start < TILE_E ? t.s1 - start : TILE_E);
    const uint64_t f0 = toff[b] & MSD_ELEM_MASK;
    const idx_t SENT = tie_sentinel<idx_t>();
    PAR(tid) {
        for (uint32_t e = tid; e < cnt; e += K_BLOCK_DIM) {
            const uint64_t p = start + e;
            const bool tp = LCP[p] == SENT;                  // (a segment head never carries the sentinel)
            const bool tn = p + 1 < t.s1 && LCP[p + 1] == SENT;
            const bool member = tp || tn;
            flags[f0 + e] = (member ? 1ull : 0ull) | (member && !tp ? 1ull << 32 : 0ull);
        }
    }
}

// ... and their copy into the work arrays: wsa[c] = SA[p], a head opens group g': seg_start[g'] = c, gpos[g'] = p
// (offs = exclusive scan of flags: members before in the low word, heads before in the high one)
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(256) msd_compact0_kernel(KCTX SegDesc sd, const uint32_t* __restrict__ ftile, const uint64_t* __restrict__ toff,
                                                 const idx_t* __restrict__ SA, const uint64_t* __restrict__ flags,
                                                 const uint64_t* __restrict__ offs, idx_t* __restrict__ wsa,
                                                 uint64_t* __restrict__ seg_start, uint64_t* __restrict__ gpos, uint32_t* __restrict__ wgid,
                                                 uint64_t* __restrict__ gdepth, uint64_t D0, uint64_t* __restrict__ gplen)
{
    // gplen[g] = the size of the group this one was split off from (0: none): a group as large as its parent made no progress
    // wgid[c] = the member's group (heads before it, itself included); gdepth[g] = D0: the chars the group's members are known to share
    const uint32_t b = ftile[K_BLOCK_IDX];
    const TileInfo t = tile_info(sd, b);
    const uint64_t start = t.s0 + (uint64_t)t.tl * TILE_E;
    const uint32_t cnt = (uint32_t)(t.s1 - start < TILE_E ? t.s1 - start : TILE_E);
    const uint64_t f0 = toff[b] & MSD_ELEM_MASK;
    PAR(tid) {
        for (uint32_t e = tid; e < cnt; e += K_BLOCK_DIM) {
            const uint64_t f = flags[f0 + e];
            if (f & 1u) {
                const uint64_t o = offs[f0 + e], c = o & 0xFFFFFFFFull;
                wsa[c] = SA[start + e];
                wgid[c] = (uint32_t)((o >> 32) + (f >> 32)) - 1u;
                if (f >> 32) { seg_start[o >> 32] = c; gpos[o >> 32] = start + e; gdepth[o >> 32] = D0; gplen[o >> 32] = 0; }
            }
        }
    }
}

// closes a group table: seg_start[G] = m, out3 = {G, m, 0, 0, 0} (total = offs[count]: members | groups << 32)
GLOBAL_FN LAUNCH_BOUNDS(64) msd_close_kernel(KCTX const uint64_t* __restrict__ total, uint64_t* __restrict__ seg_start, uint64_t* __restrict__ out3)
{
    PAR(tid) {
        if (tid == 0 && K_BLOCK_IDX == 0) {
            const uint64_t m = total[0] & 0xFFFFFFFFull, G = total[0] >> 32;
            seg_start[G] = m;
            out3[0] = G;
            out3[1] = m;
            out3[2] = 0;                               // groups larger than MSD_FIN_MAX (msd_finish_kernel counts them),
            out3[3] = 0;                               //   the largest of them,
            out3[4] = 0;                               //   (the same count: they are sorted tile by tile),
            out3[5] = 0;                               //   members listed for msd_finish_kernel,
            out3[6] = out3[7] = out3[8] = 0;           //   groups listed for msd_quick_kernel, by capacity class
        }
    }
}

// ---- one level.  Everything below is one THREAD per member of the work array (wgid: its group; skip[g] != 0: the group is
// finished -- its members are dead weight until the next compaction drops them).
constexpr uint32_t MSD_QK_MAX = TILE_E;       // groups up to this size are finished in LDS (msd_quick_kernel); only larger ones see another level
// (three capacities, so that small groups do not occupy a compute unit each: 8 / 32 / 128 KB of LDS per workgroup)
constexpr uint32_t MSD_QK_CAP[3] = {TILE_E / 16, TILE_E / 4, TILE_E};
constexpr uint32_t MSD_QK_NT[3] = {TILE_NT / 4, TILE_NT / 4, TILE_NT};

// key = the KCH chars behind the D known-equal ones
template <typename idx_t, int BITS>
GLOBAL_FN LAUNCH_BOUNDS(256) msd_rekey_kernel(KCTX const uint32_t* __restrict__ P, uint64_t n, const uint64_t* __restrict__ gdepth, uint64_t m,
                                              const uint32_t* __restrict__ wgid, const uint8_t* __restrict__ skip,
                                              const idx_t* __restrict__ wsa, uint64_t* __restrict__ wkey)
{
    PAR(tid) {
        const uint64_t i = (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (i < m && !skip[wgid[i]]) {
            const uint64_t pos = (uint64_t)wsa[i] + gdepth[wgid[i]];
            wkey[i] = pos < n ? window64<BITS>(P, pos) : 0;       // (a suffix that has ended: the pad, the smallest key)
        }
    }
}

// The groups sorted by (key, position descending): what is settled goes to SA / LCP, what is not is flagged for the next level.
template <typename idx_t, int BITS>
GLOBAL_FN LAUNCH_BOUNDS(256) msd_classify_kernel(KCTX uint64_t n, const uint64_t* __restrict__ gdepth, uint64_t m, const uint64_t* __restrict__ seg_start,
                                                 const uint32_t* __restrict__ wgid, const uint8_t* __restrict__ skip,
                                                 const uint64_t* __restrict__ key, const idx_t* __restrict__ sa,
                                                 const uint64_t* __restrict__ gpos, idx_t* __restrict__ SA, idx_t* __restrict__ LCP,
                                                 uint64_t* __restrict__ flags)
{
    PAR(tid) {
        const uint64_t i = (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (i < m) {
            const uint32_t g = wgid[i];
            uint64_t f = 0;
            if (!skip[g]) {
                const uint64_t s0 = seg_start[g], s1 = seg_start[g + 1], D = gdepth[g];
                const uint64_t k = key[i], a = (uint64_t)sa[i];
                const uint64_t pos = gpos[g] + (i - s0);
                bool tp = false;
                SA[pos] = (idx_t)a;
                if (i > s0) {
                    const uint64_t kp = key[i - 1], ap = (uint64_t)sa[i - 1];
                    if (kp != k) {
                        const uint64_t l = D + (uint32_t)caps_clz64(kp ^ k) / BITS, room = n - (a > ap ? a : ap);
                        LCP[pos] = (idx_t)(l < room ? l : room);
                    } else if (msd_ending<BITS>(n, ap, D)) LCP[pos] = (idx_t)(n - ap);     // the upper one is a prefix of this one
                    else tp = true;
                }
                const bool tn = i + 1 < s1 && key[i + 1] == k && !msd_ending<BITS>(n, a, D);
                const bool member = tp || tn;
                f = (member ? 1ull : 0ull) | (member && !tp ? 1ull << 32 : 0ull);
            }
            flags[i] = f;
        }
    }
}

// ... and its members move on (as msd_compact0_kernel, from the sorted work arrays; wgid_out may not alias wgid)
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(256) msd_compact_kernel(KCTX uint64_t m, const uint64_t* __restrict__ seg_in, const uint32_t* __restrict__ wgid,
                                                const idx_t* __restrict__ sa, const uint64_t* __restrict__ flags,
                                                const uint64_t* __restrict__ offs, const uint64_t* __restrict__ gpos_in,
                                                idx_t* __restrict__ wsa, uint64_t* __restrict__ seg_start, uint64_t* __restrict__ gpos,
                                                uint32_t* __restrict__ wgid_out, const uint64_t* __restrict__ gdepth_in,
                                                uint64_t* __restrict__ gdepth, uint32_t kch, uint64_t* __restrict__ gplen)
{
    PAR(tid) {
        const uint64_t i = (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (i < m) {
            const uint64_t f = flags[i];
            if (f & 1u) {
                const uint32_t g = wgid[i];
                const uint64_t o = offs[i], c = o & 0xFFFFFFFFull;
                wsa[c] = sa[i];
                wgid_out[c] = (uint32_t)((o >> 32) + (f >> 32)) - 1u;
                if (f >> 32) { seg_start[o >> 32] = c; gpos[o >> 32] = gpos_in[g] + (i - seg_in[g]); gdepth[o >> 32] = gdepth_in[g] + kch; gplen[o >> 32] = seg_in[g + 1] - seg_in[g]; }
            }
        }
    }
}

// A group that came out of a level as large as it went in: its members agree far beyond the next window (copies of a long exact
// repeat, suffixes at one offset of equally long letter runs: 32 chars per level would take thousands of levels).  Its depth jumps to
// what ALL its members share: msd_jump_kernel -- one thread per member, its common prefix with the group's first member from the
// known depth on (deep_scan: a periodic stretch costs one step), the minimum per group in gmin (stored inverted: an atomic
// max; preset to 0) -- then msd_jump_apply_kernel rounds it down to whole windows.
template <typename idx_t, int BITS, bool RUNS>
GLOBAL_FN LAUNCH_BOUNDS(256) msd_jump_kernel(KCTX const uint32_t* __restrict__ P, uint64_t n, uint64_t m, const uint64_t* __restrict__ seg_start,
                                             const uint32_t* __restrict__ wgid, const uint8_t* __restrict__ skip, const idx_t* __restrict__ wsa,
                                             const uint64_t* __restrict__ gdepth, const uint64_t* __restrict__ gplen, uint64_t* __restrict__ gmin)
{
    PAR(tid) {
        const uint64_t i = (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (i < m) {
            const uint32_t g = wgid[i];
            const uint64_t s0 = seg_start[g];
            if (!skip[g] && i != s0 && seg_start[g + 1] - s0 == gplen[g]) {
                const uint64_t l = deep_lcp<BITS, RUNS>(P, n, (uint64_t)wsa[s0], (uint64_t)wsa[i], gdepth[g]);
                ATOMIC_MAX_U64(&gmin[g], ~l);
            }
        }
    }
}
GLOBAL_FN LAUNCH_BOUNDS(256) msd_jump_apply_kernel(KCTX const uint64_t* __restrict__ out3, const uint8_t* __restrict__ skip,
                                                   const uint64_t* __restrict__ gmin, uint32_t kch, uint64_t* __restrict__ gdepth)
{
    const uint64_t G = out3[0];
    PAR(tid) {
        for (uint64_t g = (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid; g < G; g += (uint64_t)K_GRID_DIM * K_BLOCK_DIM) {
            if (!skip[g] && gmin[g]) {
                const uint64_t d = (~gmin[g] / kch) * kch;
                if (d > gdepth[g]) gdepth[g] = d;
            }
        }
    }
}

// The two ends of every level-0 group.  The LCP at a group's head (with the suffix before the group) and the LCP of the suffix
// behind the group were emitted by the sort from the members that stood there THEN; they depend on the member only through its
// length (all members share the key) -- but a member whose suffix ends inside the key is shorter than that, and the stable merges
// may have left it anywhere.  edges[2g], edges[2g + 1] = the group's first position and the one behind it; once every group is
// in its final order both LCPs are taken from the text again (two suffixes with different keys: one window).
GLOBAL_FN LAUNCH_BOUNDS(256) msd_edges_kernel(KCTX const uint64_t* __restrict__ seg_start, const uint64_t* __restrict__ gpos,
                                              const uint64_t* __restrict__ out3, uint64_t* __restrict__ edges)
{
    const uint64_t G = out3[0];
    PAR(tid) {
        for (uint64_t g = (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid; g < G; g += (uint64_t)K_GRID_DIM * K_BLOCK_DIM) {
            edges[2 * g] = gpos[g];
            edges[2 * g + 1] = gpos[g] + (seg_start[g + 1] - seg_start[g]);
        }
    }
}
template <typename idx_t, int BITS>
GLOBAL_FN LAUNCH_BOUNDS(256) msd_fix_edges_kernel(KCTX const uint32_t* __restrict__ P, uint64_t n, const uint64_t* __restrict__ edges, uint64_t count,
                                                  uint64_t total, const idx_t* __restrict__ SA, idx_t* __restrict__ LCP)
{
    PAR(tid) {
        const uint64_t i = (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid;
        if (i < count) {
            const uint64_t p = edges[i];
            if (p > 0 && p < total) LCP[p] = (idx_t)deep_lcp<BITS, false>(P, n, (uint64_t)SA[p - 1], (uint64_t)SA[p], 0);
        }
    }
}

// The groups of a level, one thread each.  At most MSD_FIN_MAX members: listed for msd_finish_kernel (flist: the indices of its
// members, out3[5] of them in all).  At most MSD_QK_MAX: listed for msd_quick_kernel by capacity class (qlist[c]: the group,
// out3[6 + c] of them).  Both are
// taken out (skip[g] = skip_tiles[g] = 1).  Larger ones go through another level: out3[2] = out3[4] counts them, out3[3] = the largest.
GLOBAL_FN LAUNCH_BOUNDS(256) msd_groups_kernel(KCTX const uint64_t* __restrict__ seg_start, uint8_t* __restrict__ skip, uint8_t* __restrict__ skip_tiles,
                                               uint32_t* __restrict__ flist, uint32_t* __restrict__ qlist0, uint32_t* __restrict__ qlist1,
                                               uint32_t* __restrict__ qlist2, uint64_t* __restrict__ out3)
{
    // (a workgroup reserves its share of the lists and adds its counts with ONE global atomic each: a million groups bumping the
    // counters one by one took longer than finishing them)
    SHARED_ARRAY(uint32_t, acc, 6);            // [0] members listed by this workgroup, [1] larger groups, [2] the largest, [3..5] groups per quick class
    SHARED_ARRAY(uint64_t, at0, 4);
    const uint64_t G = out3[0];
    for (uint64_t gb = (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM; gb < G; gb += (uint64_t)K_GRID_DIM * K_BLOCK_DIM) {
        TL_DECL(uint32_t, mine, 1);
        TL_DECL(uint32_t, mineq, 1);
        PAR(tid) { if (tid < 6) acc[tid] = 0; }
        SYNC();
        PAR(tid) {
            const uint64_t g = gb + tid;
            TL(mine, tid, 0) = ~0u;
            TL(mineq, tid, 0) = ~0u;
            if (g < G) {
                const uint64_t len = seg_start[g + 1] - seg_start[g];
                if (len <= MSD_QK_MAX) {
                    if (len <= MSD_FIN_MAX) TL(mine, tid, 0) = FETCH_ADD_U32(&acc[0], (uint32_t)len);
                    else {
                        const uint32_t c = len <= MSD_QK_CAP[0] ? 0u : len <= MSD_QK_CAP[1] ? 1u : 2u;
                        TL(mineq, tid, 0) = FETCH_ADD_U32(&acc[3 + c], 1u) | (c << 30);
                    }
                    skip[g] = 1;
                    skip_tiles[g] = 1;
                } else {
                    skip[g] = 0;
                    skip_tiles[g] = 0;
                    FETCH_ADD_U32(&acc[1], 1u);
                    ATOMIC_MAX_U32(&acc[2], (uint32_t)(len < 0xFFFFFFFFull ? len : 0xFFFFFFFFull));
                }
            }
        }
        SYNC();
        PAR(tid) {
            if (tid == 0) {
                at0[0] = acc[0] ? FETCH_ADD_U64(&out3[5], (uint64_t)acc[0]) : 0;
                for (uint32_t c = 0; c < 3; ++c) at0[1 + c] = acc[3 + c] ? FETCH_ADD_U64(&out3[6 + c], (uint64_t)acc[3 + c]) : 0;
                if (acc[1]) { ATOMIC_ADD_U64(&out3[2], (uint64_t)acc[1]); ATOMIC_ADD_U64(&out3[4], (uint64_t)acc[1]); }
                if (acc[2]) ATOMIC_MAX_U64(&out3[3], (uint64_t)acc[2]);
            }
        }
        SYNC();
        PAR(tid) {
            const uint64_t g = gb + tid;
            if (g < G && TL(mine, tid, 0) != ~0u) {
                const uint64_t s0 = seg_start[g], len = seg_start[g + 1] - s0, at = at0[0] + TL(mine, tid, 0);
                for (uint64_t k = 0; k < len; ++k) flist[at + k] = (uint32_t)(s0 + k);
            }
            if (g < G && TL(mineq, tid, 0) != ~0u) {
                const uint32_t c = TL(mineq, tid, 0) >> 30, at = TL(mineq, tid, 0) & 0x3FFFFFFFu;
                (c == 0 ? qlist0 : c == 1 ? qlist1 : qlist2)[at0[1 + c] + at] = (uint32_t)g;
            }
        }
        SYNC();
    }
}

// The listed groups are finished by direct comparison: MSD_FIN_LANES threads per member share the other members of its group (the
// comparisons of a member in flight together: a compare is a chain of dependent reads of the text), each compares from depth D
// on (deep_scan: run-table aware, any depth); the member's rank is the number of smaller ones, its LCP the largest one it shares
// with a smaller one (the predecessor's).  The head's LCP with ITS predecessor stands.
constexpr uint32_t MSD_FIN_LANES = 8;
constexpr uint32_t MSD_FIN_NT = 256, MSD_FIN_MEMBERS = MSD_FIN_NT / MSD_FIN_LANES;
template <typename idx_t, int BITS, bool RUNS>
GLOBAL_FN LAUNCH_BOUNDS(MSD_FIN_NT) msd_finish_kernel(KCTX const uint32_t* __restrict__ P, uint64_t n, const uint64_t* __restrict__ gdepth, const uint64_t* __restrict__ seg_start,
                                               const uint64_t* __restrict__ gpos, const idx_t* __restrict__ wsa, const uint32_t* __restrict__ wgid,
                                               const uint32_t* __restrict__ flist, idx_t* __restrict__ SA, idx_t* __restrict__ LCP,
                                               const uint64_t* __restrict__ out3)
{
    SHARED_ARRAY(uint32_t, rk, MSD_FIN_MEMBERS);
    SHARED_ARRAY(uint64_t, best, MSD_FIN_MEMBERS);
    const uint64_t m = out3[5];
    for (uint64_t base = (uint64_t)K_BLOCK_IDX * MSD_FIN_MEMBERS; base < m; base += (uint64_t)K_GRID_DIM * MSD_FIN_MEMBERS) {
        PAR(tid) { if (tid < MSD_FIN_MEMBERS) { rk[tid] = 0; best[tid] = 0; } }
        SYNC();
        PAR(tid) {
            const uint32_t q = tid / MSD_FIN_LANES, lane = tid % MSD_FIN_LANES;
            if (base + q < m) {
                const uint64_t i = flist[base + q];
                const uint32_t g = wgid[i];
                const uint64_t s0 = seg_start[g], len = seg_start[g + 1] - s0, D = gdepth[g];
                const uint64_t a = (uint64_t)wsa[i];
                uint32_t cnt = 0;
                uint64_t bl = 0;
                for (uint64_t j = s0 + lane; j < s0 + len; j += MSD_FIN_LANES) {
                    if (j == i) continue;
                    const uint64_t c = (uint64_t)wsa[j];
                    const uint64_t maxlen = n - (a > c ? a : c);
                    uint64_t wa = 0, wc = 0;
                    uint64_t l = deep_scan<BITS, RUNS>(P, n, c, a, D, maxlen, wc, wa);
                    const bool c_first = l < maxlen ? wc < wa : c > a;         // (one a prefix of the other: the shorter first)
                    l = l < maxlen ? l : maxlen;
                    if (c_first) { ++cnt; bl = l > bl ? l : bl; }
                }
                if (cnt) { FETCH_ADD_U32(&rk[q], cnt); ATOMIC_MAX_LDS_U64(&best[q], bl); }
            }
        }
        SYNC();
        PAR(tid) {
            if (tid < MSD_FIN_MEMBERS && base + tid < m) {
                const uint64_t i = flist[base + tid];
                const uint64_t p = gpos[wgid[i]] + rk[tid];
                SA[p] = wsa[i];
                if (rk[tid]) LCP[p] = (idx_t)best[tid];
            }
        }
        SYNC();                                        // rk / best are free for the next batch
    }
}

// A group of at most MSD_QK_MAX members, finished in ONE launch: multikey quicksort in LDS, every level of the refinement without a
// trip through global memory but the windows of the text.  The workgroup holds the group's positions; a SUBSEGMENT is a run of
// them known to share D0 + lvl windows (at first: the whole group, lvl 0).  Every round, every open subsegment is split three
// ways around its first member's window at that depth: smaller | equal | larger (a member whose suffix ends inside the window is
// a prefix of the others: by position, the shorter first).  The equal part moves on to the next window, the other two are
// split again at the same depth; a part of one member is settled.  A subsegment that comes out whole (all windows equal) jumps
// to what all its members share (deep_lcp: a periodic stretch is one step).  The LCP of a member with its predecessor follows
// from the round that separated the two: the depth of that round + what their windows there share (sep[i]: its level).
// Replaces ~45 launches-and-syncs deep level loops over the thousands of groups of a tandem array (25 of 119 ms on the
// GRCh38-shaped workload) by one kernel.  Every round waits for the text once (one workgroup: ~2 us), so the compute unit
// must hold several groups: capacities of 256 / 1024 / 4096 members (MSD_QK_CAP: 8 / 32 / 128 KB of LDS).
constexpr uint32_t MSD_QK_SHIFT = 21;             // cnt[start] = smaller | equal << 21 | larger << 42
constexpr uint32_t MSD_QK_MASK = (1u << MSD_QK_SHIFT) - 1u;
constexpr uint32_t MSD_QK_WHOLE = 1u << 31;       // (in a member's class | rank << 2 word)
static_assert(TILE_E < (1u << MSD_QK_SHIFT) && TILE_E <= 65535, "counts fit their fields, subsegment starts fit 16 bits");
template <typename idx_t, int BITS, bool RUNS, uint32_t CAP, uint32_t NT>
GLOBAL_FN LAUNCH_BOUNDS(NT) msd_quick_kernel(KCTX const uint32_t* __restrict__ P, uint64_t n, const uint32_t* __restrict__ qlist,
                                                  const uint64_t* __restrict__ seg_start, const uint64_t* __restrict__ gpos,
                                                  const uint64_t* __restrict__ gdepth, const idx_t* __restrict__ wsa, idx_t* __restrict__ SA,
                                                  idx_t* __restrict__ LCP)
{
    constexpr uint32_t KCH = TextTraits<BITS>::KCH, EPT = CAP / NT;
    static_assert(CAP % NT == 0 && CAP <= MSD_QK_MAX, "capacity classes");
    SHARED_ARRAY(idx_t, ssa, CAP);
    SHARED_ARRAY(uint16_t, sid, CAP);          // the start of the member's subsegment
    SHARED_ARRAY(uint16_t, slen, CAP);         // [start] members (1: settled)
    SHARED_ARRAY(uint32_t, slvl, CAP);         // [start] windows behind D0 its members are known to share
    SHARED_ARRAY(uint32_t, sep, CAP);          // [i] the level of the round that separated member i from member i - 1
    SHARED_ARRAY(uint64_t, cnt, CAP);          // [start] the three counts of a round (zero between rounds)
    SHARED_ARRAY(uint64_t, jacc, CAP / 2);     // [start / 2] what a subsegment that came out whole shares, inverted minimum (zero between rounds;
                                               //   an open subsegment has two members at least: start / 2 is its own)
    SHARED_ARRAY(uint32_t, open, 2);           // [round & 1] a subsegment of two or more members is left
    TL_DECL(idx_t, ra, EPT);
    TL_DECL(idx_t, rp, EPT);                 // the first member of the subsegment this round (the one the others are compared with)
    TL_DECL(uint32_t, rs, EPT);              // the member's subsegment (start), ~0: settled
    TL_DECL(uint32_t, rc, EPT);              // class | rank << 2 | MSD_QK_WHOLE
    TL_DECL(uint32_t, rl, EPT);              // the subsegment's level in this round
    const uint32_t g = qlist[K_BLOCK_IDX];
    const uint64_t s0 = seg_start[g], D0 = gdepth[g], p0 = gpos[g];
    const uint32_t N = (uint32_t)(seg_start[g + 1] - s0);
    PAR(tid) {
        for (uint32_t e = tid; e < N; e += NT) { ssa[e] = wsa[s0 + e]; sid[e] = 0; sep[e] = 0; cnt[e] = 0; jacc[e >> 1] = 0; }
        if (tid == 0) { slen[0] = (uint16_t)N; slvl[0] = 0; open[0] = 0; open[1] = N >= 2 ? 1u : 0u; }
    }
    // Three barriers per round (a round is as long as its trip to the text and its barriers: the launch lasts as long as its deepest
    // group, hundreds of rounds): every member fetches its own window AND the first member's (no hand-over through LDS), classes,
    // moves and records share a phase (everything they read was read before the barrier in front of them).
    for (uint32_t round = 0;; ++round) {
        SYNC();
        if (open[(round + 1u) & 1u] == 0) break;                               // block-uniform; set in the round before (or at the start)
        PAR(tid) {                                 // 1: windows, class, rank inside the class (one LDS atomic per member)
            if (tid == 0) open[round & 1u] = 0;                                //    (this round's flag: last read two barriers ago)
            UNROLL
            for (uint32_t k = 0; k < EPT; ++k) {
                const uint32_t e = tid + k * NT;
                TL(rs, tid, k) = ~0u;
                if (e < N) {
                    const uint32_t s = sid[e];
                    if (slen[s] >= 2) {
                        const uint32_t lvl = slvl[s];
                        const idx_t a = ssa[e], apx = ssa[s];
                        const uint64_t depth = D0 + (uint64_t)lvl * KCH, ap = (uint64_t)apx;
                        const uint64_t pa = (uint64_t)a + depth, pp = ap + depth;
                        const uint64_t key = pa < n ? window64<BITS>(P, pa) : 0, kp = pp < n ? window64<BITS>(P, pp) : 0;
                        uint32_t c = 1;
                        if (e != s) {
                            if (key != kp) c = key < kp ? 0u : 2u;
                            else if (msd_ending<BITS>(n, (uint64_t)a, depth) || msd_ending<BITS>(n, ap, depth)) c = (uint64_t)a > ap ? 0u : 2u;
                        }
                        const uint64_t old = FETCH_ADD_U64(&cnt[s], 1ull << (MSD_QK_SHIFT * c));
                        TL(ra, tid, k) = a;
                        TL(rp, tid, k) = apx;
                        TL(rs, tid, k) = s;
                        TL(rl, tid, k) = lvl;
                        TL(rc, tid, k) = c | ((uint32_t)((old >> (MSD_QK_SHIFT * c)) & MSD_QK_MASK) << 2);
                    }
                }
            }
        }
        SYNC();
        PAR(tid) {                                 // 2: the members move to their classes; the first of every class opens the class's record; a
            UNROLL                                 //    subsegment that came out whole measures what its members share with its first one
            for (uint32_t k = 0; k < EPT; ++k) {
                const uint32_t s = TL(rs, tid + 0u, k);
                if (s == ~0u) continue;
                const uint64_t pk = cnt[s];
                const uint32_t n0 = (uint32_t)(pk & MSD_QK_MASK), n1 = (uint32_t)((pk >> MSD_QK_SHIFT) & MSD_QK_MASK), n2 = (uint32_t)(pk >> (2 * MSD_QK_SHIFT));
                const uint32_t c = TL(rc, tid, k) & 3u, r = (TL(rc, tid, k) >> 2) & MSD_QK_MASK, lvl = TL(rl, tid, k);
                const uint32_t base = s + (c == 0 ? 0u : c == 1 ? n0 : n0 + n1);
                ssa[base + r] = TL(ra, tid, k);
                sid[base + r] = (uint16_t)base;
                if (r == 0) {
                    const uint32_t nc = c == 0 ? n0 : c == 1 ? n1 : n2;
                    slen[base] = (uint16_t)nc;
                    slvl[base] = lvl + (c == 1 ? 1u : 0u);
                    if (base != s) sep[base] = lvl;
                    if (nc >= 2) open[round & 1u] = 1;
                }
                if (n0 == 0 && n2 == 0 && n1 >= 2) {
                    TL(rc, tid, k) |= MSD_QK_WHOLE;
                    const uint64_t a = (uint64_t)TL(ra, tid, k), ap = (uint64_t)TL(rp, tid, k);
                    if (a != ap) {
                        const uint64_t l = deep_lcp<BITS, RUNS>(P, n, ap, a, D0 + ((uint64_t)lvl + 1u) * KCH);
                        ATOMIC_MAX_LDS_U64(&jacc[s >> 1], ~((l - D0) / KCH));                    // (the minimum, inverted)
                    }
                }
            }
        }
        SYNC();
        PAR(tid) {                                 // 3: ... and jumps there; the counters are zero again
            UNROLL
            for (uint32_t k = 0; k < EPT; ++k) {
                const uint32_t s = TL(rs, tid, k), e = tid + k * NT;
                if (s != ~0u && e == s) {
                    cnt[s] = 0;
                    if ((TL(rc, tid, k) & MSD_QK_WHOLE) && jacc[s >> 1]) {
                        const uint64_t w = ~jacc[s >> 1];
                        jacc[s >> 1] = 0;
                        if (w > slvl[s]) slvl[s] = (uint32_t)(w < 0xFFFFFFFFull ? w : 0xFFFFFFFFull);
                    }
                }
            }
        }
    }
    PAR(tid) {                                     // the group in its final order: SA, and the LCPs from the separating rounds
        for (uint32_t e = tid; e < N; e += NT) {
            const uint64_t a = (uint64_t)ssa[e];
            SA[p0 + e] = (idx_t)a;
            if (e) {
                const uint64_t b = (uint64_t)ssa[e - 1], depth = D0 + (uint64_t)sep[e] * KCH;
                const uint64_t wa = a + depth < n ? window64<BITS>(P, a + depth) : 0, wb = b + depth < n ? window64<BITS>(P, b + depth) : 0;
                const uint64_t l = depth + (wa == wb ? KCH : (uint32_t)caps_clz64(wa ^ wb) / BITS), room = n - (a > b ? a : b);
                LCP[p0 + e] = (idx_t)(l < room ? l : room);
            }
        }
    }
}

// ----------------------------------------------------------------------------------
// Multi-GPU exchange helpers.  After the all-to-all-v a rank holds, per source
// rank, that rank's sub-subarrays of the partitions it now owns; regroup_kernel moves run
// d (desc[3d] = source offset, desc[3d+1] = destination offset, desc[3d+2] = length) so
// that every partition is contiguous.  One workgroup per run.
// ----------------------------------------------------------------------------------
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(256) regroup_kernel(KCTX const uint64_t* __restrict__ desc, const uint64_t* __restrict__ in_key,
                                            const idx_t* __restrict__ in_sa, uint64_t* __restrict__ out_key,
                                            idx_t* __restrict__ out_sa)
{
    const uint64_t src = desc[3 * (uint64_t)K_BLOCK_IDX], dst = desc[3 * (uint64_t)K_BLOCK_IDX + 1],
                   len = desc[3 * (uint64_t)K_BLOCK_IDX + 2];
    PAR(tid) {
        for (uint64_t i = tid; i < len; i += K_BLOCK_DIM) {
            out_key[dst + i] = in_key[src + i];
            out_sa[dst + i] = in_sa[src + i];
        }
    }
}

// LCP of the first suffix of a rank's slice with the last suffix of the previous
// non-empty slice (the a11 boundary between GPUs).
// SA[base - 1] and SA[base] are neighbours in the suffix array but were sorted by different waves: their LCP from the text
template <typename idx_t, int BITS>
GLOBAL_FN LAUNCH_BOUNDS(64) wave_head_lcp_kernel(KCTX const uint32_t* __restrict__ P, uint64_t n, const idx_t* __restrict__ dSA,
                                                 idx_t* __restrict__ dLCP, uint64_t base)
{
    PAR(tid) {
        if (tid == 0 && K_BLOCK_IDX == 0)
            dLCP[base] = (idx_t)deep_lcp<BITS, true>(P, n, (uint64_t)dSA[base - 1], (uint64_t)dSA[base], 0);
    }
}

template <typename idx_t, int BITS>
GLOBAL_FN LAUNCH_BOUNDS(64) first_lcp_kernel(KCTX const uint32_t* __restrict__ P, uint64_t n, uint64_t prev_sa,
                                             const idx_t* __restrict__ sa, idx_t* __restrict__ lcp)
{
    PAR(tid) {
        if (tid == 0 && K_BLOCK_IDX == 0) lcp[0] = (idx_t)deep_lcp<BITS>(P, n, prev_sa, (uint64_t)sa[0], 0);
    }
}

// ----------------------------------------------------------------------------------
// Verifier (idea of the reference's never-called is_sorted,
// cpp:512-536): works on the RAW text with byte loops, independent of the packed text
// and keys.  err[0] += #violations; seen is an n-bit set for the permutation check.
// ----------------------------------------------------------------------------------
// cnt entries of SA / LCP are checked (cnt = n: the whole arrays; cnt < n: a slice of them, e.g. one rank's -- then
// "no value twice" is all the permutation check can say).  head != 0: entry 0 is the head of the suffix array (LCP 0).
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(256) verify_kernel(KCTX const int8_t* __restrict__ T, uint64_t n, const idx_t* __restrict__ SA,
                                           const idx_t* __restrict__ LCP, uint64_t cnt, uint32_t head, uint32_t* __restrict__ seen,
                                           uint64_t* __restrict__ err)
{
    PAR(tid) {
        const uint64_t stride = (uint64_t)K_GRID_DIM * K_BLOCK_DIM;
        uint64_t bad = 0;
        for (uint64_t i = (uint64_t)K_BLOCK_IDX * K_BLOCK_DIM + tid; i < cnt; i += stride) {
            const uint64_t b = SA[i];
            if (b >= n) { ++bad; continue; }
            const uint32_t bit = 1u << (b & 31);
#ifdef CAPS_EMUL
            const uint32_t old = seen[b >> 5]; seen[b >> 5] |= bit;
#else
            const uint32_t old = atomicOr(&seen[b >> 5], bit);
#endif
            if (old & bit) ++bad;
            if (i == 0) { if (head && LCP[0] != 0) ++bad; continue; }
            const uint64_t a = SA[i - 1];
            if (a >= n) continue;                        // counted by its own thread
            const uint64_t cap = n - (a > b ? a : b);
            uint64_t l = 0;
            while (l < cap && T[a + l] == T[b + l]) ++l;
            if (l != (uint64_t)LCP[i]) ++bad;
            if (l == cap) { if (a < b) ++bad; }
            else if (!(T[a + l] < T[b + l])) ++bad;
        }
        if (bad) ATOMIC_ADD_U64(&err[0], bad);
    }
}

// ---- f2: LCP values leave the device as BYTES (capi_impl.h HostCopySink) -------------------------------------------------------
// The D2H of SA and LCP is what a host-buffer build waits for (24 GB at C3: 390 of 494 ms), and LCP values are small -- mean 12 on
// random DNA, a few dozen on a genome.  out8[i] = lcp[i] if it is below 255, else 255 with (base + i) << 32 | lcp[i] appended to the
// list of exceptions (one atomic per wave; exc_count may run past exc_cap: the host then takes the whole array at full width).  The
// host widens the bytes into the caller's array while the next slice is on the link.  32-bit indices only (positions fit 32 bits).
constexpr uint32_t NARROW_PER = 16;            // consecutive values per thread: four 16-byte loads, one 16-byte store
GLOBAL_FN LAUNCH_BOUNDS(256) lcp_narrow_kernel(KCTX const uint32_t* __restrict__ lcp, uint64_t cnt, uint64_t base, uint8_t* __restrict__ out8,
                                               uint64_t* __restrict__ exc_count, uint64_t exc_cap, uint64_t* __restrict__ exc)
{
    // a workgroup reserves room on the list once per round for all its exceptions (inside a satellite array EVERY value is one: an
    // atomic per thread on the one counter would serialise millions of them)
    SHARED_ARRAY(uint32_t, bsum, 1);
    SHARED_ARRAY(uint64_t, bbase, 1);
    TL_DECL(uint32_t, v, NARROW_PER);
    TL_DECL(uint32_t, off, 1);
    const uint64_t per_round = (uint64_t)K_BLOCK_DIM * NARROW_PER, stride = (uint64_t)K_GRID_DIM * per_round;
    for (uint64_t r0 = (uint64_t)K_BLOCK_IDX * per_round; r0 < cnt; r0 += stride) {               // block-uniform
        PAR(tid) { if (tid == 0) bsum[0] = 0; }
        SYNC();
        PAR(tid) {
            const uint64_t i0 = r0 + (uint64_t)tid * NARROW_PER;
            uint32_t big = 0;
            UNROLL
            for (uint32_t k = 0; k < NARROW_PER; ++k) {
                TL(v, tid, k) = i0 + k < cnt ? lcp[i0 + k] : 0u;
                big += TL(v, tid, k) >= 255u ? 1u : 0u;
            }
            TL(off, tid, 0) = big ? FETCH_ADD_U32(&bsum[0], big) : 0u;
        }
        SYNC();
        PAR(tid) { if (tid == 0 && bsum[0]) bbase[0] = FETCH_ADD_U64(exc_count, (uint64_t)bsum[0]); }
        SYNC();
        PAR(tid) {
            const uint64_t i0 = r0 + (uint64_t)tid * NARROW_PER;
            uint64_t at = bsum[0] ? bbase[0] + TL(off, tid, 0) : 0;
            UNROLL
            for (uint32_t k = 0; k < NARROW_PER; ++k) {
                const uint32_t x = TL(v, tid, k);
                if (x >= 255u) {
                    if (at < exc_cap) exc[at] = ((base + i0 + k) << 32) | x;
                    ++at;
                }
                if (i0 + k < cnt) out8[i0 + k] = (uint8_t)(x < 255u ? x : 255u);
            }
        }
        SYNC();
    }
}

// ---- Burrows-Wheeler transform of a slice of the suffix array (capi_impl.h bwt_device, HostCopySink) ---------------------------
// out[k] = T[(SA[k] + n - 1) mod n] for k < cnt, SA pointing at rank `first`; the one thread that meets SA[k] == 0 stores first + k
// to *primary (a plain store: no other thread writes it; the caller set it to UINT64_MAX).  A pure gather, bound by the number of
// text loads in flight (the text is 3 GB at C3, far beyond the caches): every lane takes BWT_PER consecutive entries, reads them as
// one run of the SA (vector loads), issues all BWT_PER text loads before it uses any, and writes the bytes packed into words.
constexpr uint32_t BWT_PER = 16;               // entries per lane: 64 (u32) / 128 (u64) bytes of SA in, one 16-byte store out
// out + i0 has any alignment (a slice starts at any rank; a caller's pointer may be odd): the packed words are written through a
// type of alignment 1, which is defined for any address.  gfx950 still gets one global_store_dwordx4 per lane from it: global memory
// runs in the unaligned access mode under ROCm (the same holds for the LCP bytes of lcp_narrow_kernel at any slice base).
typedef uint32_t u32_any_align __attribute__((aligned(1)));
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(256) bwt_kernel(KCTX const uint8_t* __restrict__ T, uint64_t n, const idx_t* __restrict__ SA, uint64_t first,
                                        uint64_t cnt, uint8_t* __restrict__ out, uint64_t* __restrict__ primary)
{
    const uint64_t per_round = (uint64_t)K_BLOCK_DIM * BWT_PER, stride = (uint64_t)K_GRID_DIM * per_round;
    for (uint64_t r0 = (uint64_t)K_BLOCK_IDX * per_round; r0 < cnt; r0 += stride) {              // block-uniform
        PAR(tid) {
            const uint64_t i0 = r0 + (uint64_t)tid * BWT_PER;
            if (i0 + BWT_PER <= cnt) {
                uint64_t s[BWT_PER];
                uint32_t c[BWT_PER];
                UNROLL
                for (uint32_t k = 0; k < BWT_PER; ++k) s[k] = (uint64_t)STREAM_LOAD(&SA[i0 + k]);
                UNROLL
                for (uint32_t k = 0; k < BWT_PER; ++k) c[k] = T[s[k] ? s[k] - 1 : n - 1];     // all loads before any use
                UNROLL
                for (uint32_t k = 0; k < BWT_PER; ++k)
                    if (s[k] == 0) *primary = first + i0 + k;
                UNROLL
                for (uint32_t w = 0; w < BWT_PER / 4; ++w)
                    STREAM_STORE(reinterpret_cast<u32_any_align*>(out + i0) + w,
                                 c[4 * w] | (c[4 * w + 1] << 8) | (c[4 * w + 2] << 16) | (c[4 * w + 3] << 24));
            } else {
                for (uint64_t i = i0; i < cnt; ++i) {                                          // the ragged end of the slice
                    const uint64_t s = (uint64_t)SA[i];
                    out[i] = T[s ? s - 1 : n - 1];
                    if (s == 0) *primary = first + i;
                }
            }
        }
    }
}

// The same gather from the build's PACKED text (BITS-bit codes, most significant first in 32-bit words: 750 MB at C3 against the raw
// text's 3 GB) through a code -> byte table: code2byte holds the 4 bytes of a 2-bit alphabet (byte k = the letter of code k); 8-bit
// codes are the byte ^ 0x80 (pipeline.h build_lut).  What the host path's slices use (HostCopySink): measured at C3 on that path,
// build_bwt() - build() = +110 ms with it against +114 ms from the raw text (docs/HISTORY.md); bwt_device has only the raw text.
template <typename idx_t, int BITS>
GLOBAL_FN LAUNCH_BOUNDS(256) bwt_packed_kernel(KCTX const uint32_t* __restrict__ P, uint64_t n, const idx_t* __restrict__ SA, uint64_t first,
                                               uint64_t cnt, uint8_t* __restrict__ out, uint64_t* __restrict__ primary, uint32_t code2byte)
{
    constexpr uint32_t CPW = 32 / BITS;
    const uint64_t per_round = (uint64_t)K_BLOCK_DIM * BWT_PER, stride = (uint64_t)K_GRID_DIM * per_round;
    auto byte_of = [&](uint64_t pos, uint32_t word) -> uint32_t {
        const uint32_t code = (word >> (32u - BITS - (uint32_t)(pos % CPW) * BITS)) & ((1u << BITS) - 1u);
        return BITS == 2 ? (code2byte >> (8u * code)) & 0xFFu : code ^ 0x80u;
    };
    for (uint64_t r0 = (uint64_t)K_BLOCK_IDX * per_round; r0 < cnt; r0 += stride) {
        PAR(tid) {
            const uint64_t i0 = r0 + (uint64_t)tid * BWT_PER;
            if (i0 + BWT_PER <= cnt) {
                uint64_t s[BWT_PER];
                uint32_t c[BWT_PER];
                UNROLL
                for (uint32_t k = 0; k < BWT_PER; ++k) { const uint64_t v = (uint64_t)STREAM_LOAD(&SA[i0 + k]); s[k] = v ? v - 1 : n - 1; }
                UNROLL
                for (uint32_t k = 0; k < BWT_PER; ++k) c[k] = P[s[k] / CPW];
                UNROLL
                for (uint32_t k = 0; k < BWT_PER; ++k) {
                    c[k] = byte_of(s[k], c[k]);
                    if (s[k] == n - 1) *primary = first + i0 + k;        // (only SA == 0 maps to n - 1)
                }
                UNROLL
                for (uint32_t w = 0; w < BWT_PER / 4; ++w)
                    STREAM_STORE(reinterpret_cast<u32_any_align*>(out + i0) + w,
                                 c[4 * w] | (c[4 * w + 1] << 8) | (c[4 * w + 2] << 16) | (c[4 * w + 3] << 24));
            } else {
                for (uint64_t i = i0; i < cnt; ++i) {
                    const uint64_t v = (uint64_t)SA[i], q = v ? v - 1 : n - 1;
                    out[i] = (uint8_t)byte_of(q, P[q / CPW]);
                    if (v == 0) *primary = first + i;
                }
            }
        }
    }
}

// ---- inverse Burrows-Wheeler transform (capi_impl.h inverse_bwt_device) --------------------------------------------------------
// Rows r = 0 .. n of the sorted rotations of T·$: L[0] = BWT[primary], L[r] = BWT[r - 1] for 1 <= r <= primary, L[primary + 1] = '$',
// L[r] = BWT[r - 1] after that.  Symbols as keys: '$' = 0, a byte b = (b ^ 0x80) + 1 (signed-char order), IBWT_KEYS of them.
// LF[r] = C[key(L[r])] + |{r' < r : L[r'] = L[r]}|, and T[n - 1 - t] = L[LF^t(0)] = F[LF^(t+1)(0)]: a step of the walk is ONE load
// (F is the key whose row range [C[k], C[k + 1]) holds LF[r], no L is read).  The walk is cut at splitter rows (every IBWT_S0-th),
// the list of splitters ranked by walks over it (every IBWT_S1-th node, level by level, until a list fits one workgroup), and every
// segment walked again, writing its stretch of T from its offset.  Every loop is bounded by n + 1 steps (or by its list's length),
// whatever the input: LF is a permutation by construction, so a walk from a splitter meets a splitter again.
constexpr uint32_t IBWT_KEYS = 257;
constexpr uint32_t IBWT_NT = 256;              // threads of every inverse-BWT kernel (the rank masks below have IBWT_NT bits)
constexpr uint32_t IBWT_ROUNDS = 64;           // rows of a tile of the LF table: IBWT_NT * IBWT_ROUNDS
constexpr uint64_t IBWT_TILE = (uint64_t)IBWT_NT * IBWT_ROUNDS;
constexpr uint32_t IBWT_S0_LOG = 6, IBWT_S1_LOG = 6;                 // splitter spacing: rows of the LF walk, nodes of a list
constexpr uint64_t IBWT_S0 = 1ull << IBWT_S0_LOG, IBWT_S1 = 1ull << IBWT_S1_LOG;
constexpr uint32_t IBWT_TOP = 256;             // a list of at most this many nodes is ranked by one workgroup in LDS
constexpr uint32_t IBWT_Q = 4096;              // walks per workgroup range (the lanes take them one by one from an LDS counter)

HD uint32_t ibwt_key_of_row(const uint8_t* __restrict__ B, uint64_t r, uint64_t primary)
{
    if (r == primary + 1) return 0;
    return (uint32_t)(B[r ? r - 1 : primary] ^ 0x80u) + 1u;
}

// per tile of IBWT_TILE rows: how many rows hold each key -> cnt[key * n_tiles + tile] (key-major, for the scan below)
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(IBWT_NT) ibwt_count_kernel(KCTX const uint8_t* __restrict__ B, uint64_t n, uint64_t primary, uint64_t n_tiles,
                                                    idx_t* __restrict__ cnt)
{
    SHARED_ARRAY(uint32_t, h, IBWT_KEYS);
    for (uint64_t tile = K_BLOCK_IDX; tile < n_tiles; tile += K_GRID_DIM) {         // block-uniform
        PAR(tid) { for (uint32_t k = tid; k < IBWT_KEYS; k += IBWT_NT) h[k] = 0; }
        SYNC();
        PAR(tid) {
            const uint64_t r0 = tile * IBWT_TILE;
            for (uint32_t j = 0; j < IBWT_ROUNDS; ++j) {
                const uint64_t r = r0 + (uint64_t)j * IBWT_NT + tid;
                if (r <= n) FETCH_ADD_U32(&h[ibwt_key_of_row(B, r, primary)], 1u);
            }
        }
        SYNC();
        PAR(tid) { for (uint32_t k = tid; k < IBWT_KEYS; k += IBWT_NT) cnt[(uint64_t)k * n_tiles + tile] = (idx_t)h[k]; }
        SYNC();
    }
}

// one workgroup per key: cnt[key][tile] -> the exclusive prefix over the tiles, in place; total[key] = the key's rows
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(IBWT_NT) ibwt_scan_kernel(KCTX idx_t* __restrict__ cnt, uint64_t n_tiles, uint64_t* __restrict__ total)
{
    SHARED_ARRAY(uint64_t, part, IBWT_NT);
    const uint64_t per = (n_tiles + IBWT_NT - 1) / IBWT_NT;
    for (uint32_t key = K_BLOCK_IDX; key < IBWT_KEYS; key += K_GRID_DIM) {          // block-uniform
        idx_t* col = cnt + (uint64_t)key * n_tiles;
        PAR(tid) {
            const uint64_t a = std::min<uint64_t>(n_tiles, tid * per), b = std::min<uint64_t>(n_tiles, a + per);
            uint64_t s = 0;
            for (uint64_t k = a; k < b; ++k) s += (uint64_t)col[k];
            part[tid] = s;
        }
        SYNC();
        PAR(tid) {
            if (tid == 0) {
                uint64_t s = 0;
                for (uint32_t k = 0; k < IBWT_NT; ++k) { const uint64_t v = part[k]; part[k] = s; s += v; }
                total[key] = s;
            }
        }
        SYNC();
        PAR(tid) {
            const uint64_t a = std::min<uint64_t>(n_tiles, tid * per), b = std::min<uint64_t>(n_tiles, a + per);
            uint64_t s = part[tid];
            for (uint64_t k = a; k < b; ++k) { const uint64_t v = (uint64_t)col[k]; col[k] = (idx_t)s; s += v; }
        }
        SYNC();
    }
}

// one thread: C[key] (first row of the key in F, C[IBWT_KEYS] = n + 1) and the keys present, as the walk's range table:
// sym[0] = their number, then sym[1 + i] = the first row of the i-th present key | its byte << 56 ('$' first, row 0)
GLOBAL_FN LAUNCH_BOUNDS(64) ibwt_c_kernel(KCTX const uint64_t* __restrict__ total, uint64_t* __restrict__ C, uint64_t* __restrict__ sym)
{
    PAR(tid) {
        if (tid == 0) {
            uint64_t s = 0, m = 0;
            for (uint32_t k = 0; k < IBWT_KEYS; ++k) {
                C[k] = s;
                if (total[k]) sym[1 + m++] = s | ((uint64_t)(k ? ((k - 1) ^ 0x80u) : 0u) << 56);
                s += total[k];
            }
            C[IBWT_KEYS] = s;
            sym[0] = m;
        }
    }
}

// LF[r] for the rows of every tile: C[key] + the key's rows in earlier tiles (pre) + its rows before r in this tile.  The tile goes
// in rounds of IBWT_NT rows, one per thread; a thread's rank among the round's rows of its key is the number of lower bits in the
// key's IBWT_NT-bit mask (set by LDS atomics), and the round's last row of a key carries the key's count on and clears its mask.
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(IBWT_NT) ibwt_lf_kernel(KCTX const uint8_t* __restrict__ B, uint64_t n, uint64_t primary, uint64_t n_tiles,
                                                 const idx_t* __restrict__ pre, const uint64_t* __restrict__ C, idx_t* __restrict__ LF)
{
    constexpr uint32_t MW = IBWT_NT / 32;         // mask words per key
    SHARED_ARRAY(uint32_t, mask, IBWT_KEYS * MW);
    SHARED_ARRAY(uint64_t, base, IBWT_KEYS);
    TL_DECL(uint32_t, st, 2);                     // the row's key (IBWT_KEYS: no row); the key's rows in the round if last, else 0
    for (uint64_t tile = K_BLOCK_IDX; tile < n_tiles; tile += K_GRID_DIM) {         // block-uniform
        PAR(tid) {
            for (uint32_t k = tid; k < IBWT_KEYS; k += IBWT_NT) base[k] = C[k] + (uint64_t)pre[(uint64_t)k * n_tiles + tile];
            for (uint32_t w = tid; w < IBWT_KEYS * MW; w += IBWT_NT) mask[w] = 0;
        }
        SYNC();
        for (uint32_t j = 0; j < IBWT_ROUNDS; ++j) {
            const uint64_t r0 = tile * IBWT_TILE + (uint64_t)j * IBWT_NT;
            if (r0 > n) break;                                                      // block-uniform
            PAR(tid) {
                const uint64_t r = r0 + tid;
                const uint32_t key = r <= n ? ibwt_key_of_row(B, r, primary) : IBWT_KEYS;
                TL(st, tid, 0) = key;
                if (key < IBWT_KEYS) ATOMIC_OR_U32(&mask[key * MW + tid / 32], 1u << (tid % 32));
            }
            SYNC();
            PAR(tid) {
                const uint32_t key = TL(st, tid, 0);
                TL(st, tid, 1) = 0;
                if (key < IBWT_KEYS) {
                    const uint32_t* mk = mask + key * MW;
                    const uint32_t w = tid / 32, bit = tid % 32;
                    uint32_t below = 0, above = 0;
                    for (uint32_t i = 0; i < MW; ++i) {
                        const uint32_t v = mk[i];
                        if (i < w) below += (uint32_t)__builtin_popcount(v);
                        else if (i > w) above += (uint32_t)__builtin_popcount(v);
                        else {
                            below += (uint32_t)__builtin_popcount(v & ((1u << bit) - 1u));
                            above += (uint32_t)__builtin_popcount(v >> bit) - 1u;
                        }
                    }
                    const uint64_t r = r0 + tid;
                    LF[r] = (idx_t)(base[key] + below);
                    if (above == 0) TL(st, tid, 1) = below + 1;
                }
            }
            SYNC();
            PAR(tid) {
                const uint32_t key = TL(st, tid, 0), c = TL(st, tid, 1);
                if (key < IBWT_KEYS && c) {
                    base[key] += c;
                    for (uint32_t i = 0; i < MW; ++i) mask[key * MW + i] = 0;
                }
            }
            SYNC();
        }
    }
}

// The walks, one kind per MODE, over ranges of IBWT_Q walks per workgroup (a lane takes the next walk of the range from an LDS
// counter when its last one ends: walk lengths vary, roughly geometric on natural text).
//   IBWT_LINK0  from splitter row j * S0 along LF to the next splitter: succ[j], len[j] (rows; len[j] <= n + 1)
//   IBWT_LINK   the same over a list (lsucc, llen) of M nodes with splitters at every S1-th node: succ[J], len[J] = the summed weight
//   IBWT_PROP   the offsets of a list's nodes from the offsets of its splitters: loff[node] = off[J] + the weight before it
//   IBWT_WRITE  from splitter row j * S0 at offset off[j] for len[j] steps: T[n - 1 - t] = F[LF[row]] for t = off[j] .. (t < n)
enum { IBWT_LINK0 = 0, IBWT_LINK = 1, IBWT_PROP = 2, IBWT_WRITE = 3 };
template <typename idx_t, int MODE>
GLOBAL_FN LAUNCH_BOUNDS(IBWT_NT) ibwt_walk_kernel(KCTX const idx_t* __restrict__ LF, uint64_t n, uint64_t walks, uint64_t M,
                                                   const idx_t* __restrict__ lsucc, const uint64_t* __restrict__ llen, uint64_t* __restrict__ loff,
                                                   idx_t* __restrict__ succ, uint64_t* __restrict__ len, const uint64_t* __restrict__ off,
                                                   const uint64_t* __restrict__ sym, uint8_t* __restrict__ T)
{
    SHARED_ARRAY(uint32_t, q, 1);
    SHARED_ARRAY(uint64_t, bnd, IBWT_KEYS);       // IBWT_WRITE: the first rows of the present keys (sym), and their bytes
    SHARED_ARRAY(uint8_t, byt, IBWT_KEYS);
    uint32_t nsym = 0;
    if (MODE == IBWT_WRITE) {
        PAR(tid) {
            for (uint32_t k = tid; k < IBWT_KEYS; k += IBWT_NT) {
                const uint64_t v = k < sym[0] ? sym[1 + k] : ~0ull;
                bnd[k] = v & ((1ull << 56) - 1);
                byt[k] = (uint8_t)(v >> 56);
            }
        }
        SYNC();
        nsym = (uint32_t)sym[0];
    }
    const uint64_t ranges = (walks + IBWT_Q - 1) / IBWT_Q;
    const uint32_t salign = (uint32_t)((uintptr_t)T & 3u);
    for (uint64_t rg = K_BLOCK_IDX; rg < ranges; rg += K_GRID_DIM) {               // block-uniform
        PAR(tid) { if (tid == 0) q[0] = 0; }
        SYNC();
        PAR(tid) {
            const uint64_t lo = rg * IBWT_Q, cnt = std::min<uint64_t>(IBWT_Q, walks - lo);
            for (;;) {
                const uint32_t i = FETCH_ADD_U32(&q[0], 1u);
                if (i >= cnt) break;
                const uint64_t j = lo + i;
                if (MODE == IBWT_LINK0) {
                    uint64_t cur = j << IBWT_S0_LOG, steps = 0;
                    do { cur = (uint64_t)LF[cur]; ++steps; } while ((cur & (IBWT_S0 - 1)) != 0 && steps <= n);
                    succ[j] = (idx_t)(cur >> IBWT_S0_LOG);
                    len[j] = steps;
                } else if (MODE == IBWT_LINK) {
                    uint64_t cur = j << IBWT_S1_LOG, steps = 0, w = 0;
                    do { w += llen[cur]; cur = (uint64_t)lsucc[cur]; ++steps; } while ((cur & (IBWT_S1 - 1)) != 0 && steps < M);
                    succ[j] = (idx_t)(cur >> IBWT_S1_LOG);
                    len[j] = w;
                } else if (MODE == IBWT_PROP) {
                    uint64_t cur = j << IBWT_S1_LOG, steps = 0, o = off[j];
                    do { loff[cur] = o; o += llen[cur]; cur = (uint64_t)lsucc[cur]; ++steps; } while ((cur & (IBWT_S1 - 1)) != 0 && steps < M);
                } else {
                    // positions hi = n - 1 - off down to lo: a word store for a 4-byte word of T that lies inside them, byte stores at
                    // the edges (a neighbouring segment owns the rest of an edge word)
                    const uint64_t o = off[j], steps = std::min<uint64_t>(len[j], n + 1);
                    if (o > n) continue;                                            // (never, after the single-cycle check)
                    const int64_t hi = (int64_t)n - 1 - (int64_t)o, lo = std::max<int64_t>(0, hi - (int64_t)steps + 1);
                    uint64_t cur = j << IBWT_S0_LOG;
                    uint32_t word = 0;
                    for (uint64_t k = 0; k < steps; ++k) {
                        cur = (uint64_t)LF[cur];
                        const int64_t p = hi - (int64_t)k;
                        if (p < 0) break;                                           // the '$' step (t = n)
                        uint32_t a = 0, m = nsym;                                   // the last present key whose first row <= cur
                        while (m > 1) { const uint32_t h = m / 2; if (bnd[a + h] <= cur) { a += h; m -= h; } else m = h; }
                        const uint32_t c = byt[a];
                        const uint32_t qb = (uint32_t)((salign + (uint64_t)p) & 3u);
                        const int64_t ws = p - (int64_t)qb;
                        if (ws >= lo && ws + 3 <= hi) {
                            word |= c << (8 * qb);
                            if (qb == 0) { *reinterpret_cast<uint32_t*>(T + ws) = word; word = 0; }
                        } else T[p] = (uint8_t)c;
                    }
                }
            }
        }
        SYNC();
    }
}

// The top list (M <= IBWT_TOP nodes) in LDS, walked by one thread from node 0: off[node] = the rows before it on the cycle of row 0.
// res[0] = 1 when that cycle holds every row (it comes back to node 0 with n + 1 rows: LF is one cycle, the input a BWT), else 0;
// res[1] = the rows counted, res[2] = the nodes visited.
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(IBWT_NT) ibwt_top_kernel(KCTX const idx_t* __restrict__ succ, const uint64_t* __restrict__ len, uint64_t M,
                                                  uint64_t n, uint64_t* __restrict__ off, uint64_t* __restrict__ res)
{
    SHARED_ARRAY(uint32_t, s, IBWT_TOP);
    SHARED_ARRAY(uint64_t, w, IBWT_TOP);
    SHARED_ARRAY(uint64_t, o, IBWT_TOP);
    PAR(tid) {
        for (uint32_t k = tid; k < IBWT_TOP; k += IBWT_NT) {
            s[k] = k < M ? (uint32_t)succ[k] : 0u;
            w[k] = k < M ? len[k] : 0;
            o[k] = 0;
        }
    }
    SYNC();
    PAR(tid) {
        if (tid == 0) {
            uint64_t acc = 0, steps = 0;
            uint32_t cur = 0;
            do { o[cur] = acc; acc += w[cur]; cur = s[cur]; ++steps; } while (cur != 0 && steps < M);
            res[0] = cur == 0 && acc == n + 1 ? 1 : 0;
            res[1] = acc;
            res[2] = steps;
        }
    }
    SYNC();
    PAR(tid) { for (uint32_t k = tid; k < M; k += IBWT_NT) off[k] = o[k]; }
}

// ---- FM-index over (BWT, primary) (capi_impl.h fm_*; include/caps_sa_hip.h "FM-index") ------------------------------------------
// Rows and L as in the inverse BWT above.  The alphabet has at most 4 bytes, coded 0 .. sigma - 1 in signed-char order; the '$' row
// stores code 0 and Occ(0, r) gives one back for r > primary + 1.  The Occ section is an array of blocks of ROWS rows, one aligned
// block = the 4 absolute counts (idx_t: symbols of each code in the rows before the block), the rows' 2-bit codes (row j of a
// word at bits 2j) and one "this row's SA value is sampled" bit per row:
//   _u32   64 B per 128 rows: counts 16 B | codes 32 B | marks 16 B        _u64  128 B per 256 rows: 32 B | 64 B | 32 B
// so Occ(c, r), the code of row r and its mark are ONE block: a step of a query is one line.  C[c] = the first row whose rotation
// starts with code c (C[0] = 1: row 0 starts with '$'), C[4] = n + 1.  Samples: the SA values that are multiples of s, in row
// order; the sample of a marked row = samples[mrank[block] + marks below the row in its block].
// The query kernels take the header's fields by value (FmView: validated on the host) and compare every row, block and sample
// index with its section's size before it becomes an address: whatever the body holds, they read inside the blob and end.
constexpr uint32_t FM_NT = 256;                // threads of every FM kernel
constexpr uint32_t FM_WROWS = 16;              // rows of a code word
constexpr uint32_t FM_ROUNDS = 4;              // code words per thread and tile
constexpr uint64_t FM_TILE = (uint64_t)FM_NT * FM_WROWS * FM_ROUNDS;      // rows of a tile: 16,384 (a whole number of blocks)
constexpr uint32_t FM_MROWS = 32, FM_MROUNDS = 2;                         // mark pass: rows per thread (one mark word), rounds per tile
constexpr uint32_t FM_KEYS = 5;                // columns of the tile counts: the 4 codes, the marks
constexpr uint32_t FM_MAX_SAMPLE = 1024;
template <typename idx_t> struct FmGeom {
    static constexpr uint32_t ROWS = sizeof(idx_t) == 4 ? 128u : 256u;    // rows of a block
    static constexpr uint32_t BW = ROWS / 8;                              // 32-bit words of a block (16 / 32)
    static constexpr uint32_t CW0 = sizeof(idx_t);                        // first code word (behind 4 counts of idx_t)
    static constexpr uint32_t CWN = ROWS / 16;                            // code words
    static constexpr uint32_t MW0 = CW0 + CWN;                            // first mark word
    static constexpr uint32_t MWN = ROWS / 32;                            // mark words
};
struct FmView {
    uint64_t n, primary;
    uint64_t C[5];
    uint64_t n_blocks, n_samples;
    const uint32_t* occ;
    const void* mrank;                         // idx_t[n_blocks]
    const void* samples;                       // idx_t[n_samples]
    uint32_t sigma, syms, s;                   // syms: byte k = the letter of code k
    // format version 2 (else null, 0, 0): rowof[k] = the row of the suffix at text position k * t, idx_t[n_text_samples]
    const void* rowof;
    uint64_t n_text_samples;
    uint32_t t;
};

// the code of byte b under the alphabet (syms, sigma): the number of letters below it in signed-char order (b need not be a letter)
HD uint32_t fm_code_of(uint32_t syms, uint32_t sigma, uint32_t b)
{
    const uint32_t kb = b ^ 0x80u;
    uint32_t c = 0;
    UNROLL
    for (uint32_t k = 1; k < 4; ++k) c += (k < sigma && kb >= (((syms >> (8u * k)) & 0xFFu) ^ 0x80u)) ? 1u : 0u;
    return c;
}
HD bool fm_is_letter(uint32_t syms, uint32_t sigma, uint32_t b, uint32_t c) { return c < sigma && ((syms >> (8u * c)) & 0xFFu) == b; }

// the code word of rows r0 .. r0 + 15 (r0 a multiple of 16)
HD uint32_t fm_code_word(const uint8_t* __restrict__ B, uint64_t n, uint64_t primary, uint64_t r0, uint32_t syms, uint32_t sigma)
{
    uint32_t w = 0;
    if (r0 >= FM_WROWS && r0 + FM_WROWS <= n && !(primary + 1 >= r0 && primary + 1 < r0 + FM_WROWS)) {
        // rows r0 .. r0 + 15 = bytes r0 - 1 .. r0 + 14: the 16 bytes at r0 (any alignment) and the one before them
        uint32_t x[4];
        UNROLL
        for (uint32_t k = 0; k < 4; ++k) x[k] = STREAM_LOAD(reinterpret_cast<const u32_any_align*>(B + r0) + k);
        uint32_t prev = B[r0 - 1];
        UNROLL
        for (uint32_t j = 0; j < FM_WROWS; ++j) {
            w |= fm_code_of(syms, sigma, prev) << (2u * j);
            prev = (x[j / 4] >> (8u * (j % 4))) & 0xFFu;
        }
    } else {
        for (uint32_t j = 0; j < FM_WROWS; ++j) {
            const uint64_t r = r0 + j;
            if (r > n || r == primary + 1) continue;
            w |= fm_code_of(syms, sigma, B[r ? r - 1 : primary]) << (2u * j);
        }
    }
    return w;
}
// rows of code c among the first `rows` (0 .. 16) rows of a code word
HD uint32_t fm_word_rank(uint32_t w, uint32_t c, uint32_t rows)
{
    const uint32_t x = w ^ (c * 0x55555555u);
    uint32_t m = ~(x | (x >> 1)) & 0x55555555u;
    if (rows < FM_WROWS) m &= (1u << (2u * rows)) - 1u;
    return (uint32_t)__builtin_popcount(m);
}

// alphabet probe: the set of byte values in B as 256 bits, OR-ed into present[8].  Every lane keeps the set in four 64-bit
// registers (no LDS traffic per byte: with 4 letters every LDS atomic of a wave would hit one of 4 words).
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) fm_probe_kernel(KCTX const uint8_t* __restrict__ B, uint64_t n, uint32_t* __restrict__ present)
{
    SHARED_ARRAY(uint32_t, pm, 8);
    PAR(tid) { if (tid < 8) pm[tid] = 0; }
    SYNC();
    PAR(tid) {
        uint64_t m[4] = {0, 0, 0, 0};
        auto add = [&](uint32_t b) {
            const uint64_t bit = 1ull << (b & 63u);
            const uint32_t h = b >> 6;
            m[0] |= h == 0 ? bit : 0; m[1] |= h == 1 ? bit : 0; m[2] |= h == 2 ? bit : 0; m[3] |= h == 3 ? bit : 0;
        };
        const uint64_t chunks = (n + 15) / 16, stride = (uint64_t)K_GRID_DIM * FM_NT;
        for (uint64_t ch = (uint64_t)K_BLOCK_IDX * FM_NT + tid; ch < chunks; ch += stride) {
            const uint64_t i0 = ch * 16;
            if (i0 + 16 <= n) {
                uint32_t x[4];
                UNROLL
                for (uint32_t k = 0; k < 4; ++k) x[k] = STREAM_LOAD(reinterpret_cast<const u32_any_align*>(B + i0) + k);
                UNROLL
                for (uint32_t j = 0; j < 16; ++j) add((x[j / 4] >> (8u * (j % 4))) & 0xFFu);
            } else {
                for (uint64_t i = i0; i < n; ++i) add(B[i]);
            }
        }
        for (uint32_t k = 0; k < 4; ++k) {
            if ((uint32_t)m[k]) ATOMIC_OR_U32(&pm[2 * k], (uint32_t)m[k]);
            if ((uint32_t)(m[k] >> 32)) ATOMIC_OR_U32(&pm[2 * k + 1], (uint32_t)(m[k] >> 32));
        }
    }
    SYNC();
    PAR(tid) { if (tid < 8 && pm[tid]) ATOMIC_OR_U32(&present[tid], pm[tid]); }
}

// per tile of FM_TILE rows: the rows of each code -> cnt[code * n_tiles + tile] (the '$' row and the rows behind n count as code 0:
// they are stored so)
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) fm_tile_count_kernel(KCTX const uint8_t* __restrict__ B, uint64_t n, uint64_t primary, uint64_t n_tiles,
                                                     uint32_t syms, uint32_t sigma, uint64_t* __restrict__ cnt)
{
    SHARED_ARRAY(uint32_t, h, 4);
    for (uint64_t tile = K_BLOCK_IDX; tile < n_tiles; tile += K_GRID_DIM) {         // block-uniform
        PAR(tid) { if (tid < 4) h[tid] = 0; }
        SYNC();
        PAR(tid) {
            uint32_t c[4] = {0, 0, 0, 0};
            for (uint32_t j = 0; j < FM_ROUNDS; ++j) {
                const uint64_t r0 = tile * FM_TILE + ((uint64_t)j * FM_NT + tid) * FM_WROWS;
                const uint32_t w = fm_code_word(B, n, primary, r0, syms, sigma);
                UNROLL
                for (uint32_t k = 0; k < 4; ++k) c[k] += fm_word_rank(w, k, FM_WROWS);
            }
            for (uint32_t k = 0; k < 4; ++k) if (c[k]) FETCH_ADD_U32(&h[k], c[k]);
        }
        SYNC();
        PAR(tid) { if (tid < 4) cnt[(uint64_t)tid * n_tiles + tile] = h[tid]; }
        SYNC();
    }
}

// one workgroup per column: cnt[key][tile] -> the exclusive prefix over the tiles, in place; total[key] (ibwt_scan_kernel's pattern)
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) fm_scan_kernel(KCTX uint64_t* __restrict__ cnt, uint64_t n_tiles, uint32_t key0, uint32_t keys,
                                               uint64_t* __restrict__ total)
{
    SHARED_ARRAY(uint64_t, part, FM_NT);
    const uint64_t per = (n_tiles + FM_NT - 1) / FM_NT;
    for (uint32_t key = key0 + K_BLOCK_IDX; key < key0 + keys; key += K_GRID_DIM) { // block-uniform
        uint64_t* col = cnt + (uint64_t)key * n_tiles;
        PAR(tid) {
            const uint64_t a = std::min<uint64_t>(n_tiles, tid * per), b = std::min<uint64_t>(n_tiles, a + per);
            uint64_t s = 0;
            for (uint64_t k = a; k < b; ++k) s += col[k];
            part[tid] = s;
        }
        SYNC();
        PAR(tid) {
            if (tid == 0) {
                uint64_t s = 0;
                for (uint32_t k = 0; k < FM_NT; ++k) { const uint64_t v = part[k]; part[k] = s; s += v; }
                total[key] = s;
            }
        }
        SYNC();
        PAR(tid) {
            const uint64_t a = std::min<uint64_t>(n_tiles, tid * per), b = std::min<uint64_t>(n_tiles, a + per);
            uint64_t s = part[tid];
            for (uint64_t k = a; k < b; ++k) { const uint64_t v = col[k]; col[k] = s; s += v; }
        }
        SYNC();
    }
}

// the pack pass: the blocks of every tile.  A round is FM_NT code words = FM_NT / CWN blocks: every thread makes one word and its 4
// counts, the first thread of a block sums its block's, four threads scan the blocks of the round (one code each), then the words
// and the absolute counts go out; the mark words are zeroed here (fm_mark_kernel sets them when there is an SA).
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) fm_pack_kernel(KCTX const uint8_t* __restrict__ B, uint64_t n, uint64_t primary, uint64_t n_tiles,
                                               uint64_t n_blocks, uint32_t syms, uint32_t sigma, const uint64_t* __restrict__ pre,
                                               uint32_t* __restrict__ occ)
{
    using G = FmGeom<idx_t>;
    constexpr uint32_t BPR = FM_NT / G::CWN;      // blocks of a round
    SHARED_ARRAY(uint32_t, tc, 4 * FM_NT);        // [code][thread]
    SHARED_ARRAY(uint64_t, bc, 4 * BPR);          // [code][block of the round]: the sum, then the absolute count before the block
    SHARED_ARRAY(uint64_t, run, 4);
    TL_DECL(uint32_t, wd, 1);
    for (uint64_t tile = K_BLOCK_IDX; tile < n_tiles; tile += K_GRID_DIM) {         // block-uniform
        PAR(tid) { if (tid < 4) run[tid] = pre[(uint64_t)tid * n_tiles + tile]; }
        SYNC();
        for (uint32_t j = 0; j < FM_ROUNDS; ++j) {
            const uint64_t w0 = (tile * FM_ROUNDS + j) * FM_NT;                     // first code word of the round
            PAR(tid) {
                const uint32_t w = fm_code_word(B, n, primary, (w0 + tid) * FM_WROWS, syms, sigma);
                TL(wd, tid, 0) = w;
                UNROLL
                for (uint32_t k = 0; k < 4; ++k) tc[k * FM_NT + tid] = fm_word_rank(w, k, FM_WROWS);
            }
            SYNC();
            PAR(tid) {
                if (tid % G::CWN == 0) {
                    for (uint32_t k = 0; k < 4; ++k) {
                        uint32_t s = 0;
                        for (uint32_t i = 0; i < G::CWN; ++i) s += tc[k * FM_NT + tid + i];
                        bc[k * BPR + tid / G::CWN] = s;
                    }
                }
            }
            SYNC();
            PAR(tid) {
                if (tid < 4) {
                    uint64_t s = run[tid];
                    for (uint32_t i = 0; i < BPR; ++i) { const uint64_t v = bc[tid * BPR + i]; bc[tid * BPR + i] = s; s += v; }
                    run[tid] = s;
                }
            }
            SYNC();
            PAR(tid) {
                const uint64_t blk = (w0 + tid) / G::CWN;
                if (blk < n_blocks) {
                    uint32_t* p = occ + blk * G::BW;
                    p[G::CW0 + tid % G::CWN] = TL(wd, tid, 0);
                    if (tid % G::CWN == 0) {
                        for (uint32_t k = 0; k < 4; ++k) reinterpret_cast<idx_t*>(p)[k] = (idx_t)bc[k * BPR + tid / G::CWN];
                        for (uint32_t k = 0; k < G::MWN; ++k) p[G::MW0 + k] = 0;
                    }
                }
            }
            SYNC();
        }
    }
}

// the mark word of rows r0 .. r0 + 31 (row k + 1 is SA rank k): bit j = SA[r0 + j - 1] is a multiple of s
template <typename idx_t>
HD uint32_t fm_mark_word(const idx_t* __restrict__ SA, uint64_t n, uint64_t r0, uint32_t s)
{
    uint32_t m = 0;
    if (r0 >= 1 && r0 + FM_MROWS <= n + 1) {
        UNROLL
        for (uint32_t j = 0; j < FM_MROWS; ++j) m |= (((uint64_t)STREAM_LOAD(&SA[r0 + j - 1]) & (s - 1u)) == 0 ? 1u : 0u) << j;
    } else {
        for (uint32_t j = 0; j < FM_MROWS; ++j) {
            const uint64_t r = r0 + j;
            if (r >= 1 && r <= n && ((uint64_t)SA[r - 1] & (s - 1u)) == 0) m |= 1u << j;
        }
    }
    return m;
}

// the mark pass: the mark words of every block, mrank[block] = the marks before the block IN ITS TILE, cnt[4][tile] = the tile's marks.
// FROM_OCC: the mark words stand in the blocks already (fm_walk_kernel FMW_MARK set them; SA is not read): the ranks and counts alone.
template <typename idx_t, bool FROM_OCC = false>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) fm_mark_kernel(KCTX const idx_t* __restrict__ SA, uint64_t n, uint64_t n_tiles, uint64_t n_blocks, uint32_t s,
                                               uint32_t* __restrict__ occ, idx_t* __restrict__ mrank, uint64_t* __restrict__ cnt)
{
    using G = FmGeom<idx_t>;
    constexpr uint32_t BPR = FM_NT / G::MWN;
    SHARED_ARRAY(uint32_t, tc, FM_NT);
    SHARED_ARRAY(uint32_t, bc, BPR);
    SHARED_ARRAY(uint32_t, run, 1);
    for (uint64_t tile = K_BLOCK_IDX; tile < n_tiles; tile += K_GRID_DIM) {         // block-uniform
        PAR(tid) { if (tid == 0) run[0] = 0; }
        SYNC();
        for (uint32_t j = 0; j < FM_MROUNDS; ++j) {
            const uint64_t w0 = (tile * FM_MROUNDS + j) * FM_NT;                    // first mark word of the round
            PAR(tid) {
                const uint64_t blk = (w0 + tid) / G::MWN;
                uint32_t m;
                if (FROM_OCC) m = blk < n_blocks ? occ[blk * G::BW + G::MW0 + tid % G::MWN] : 0u;
                else {
                    m = fm_mark_word<idx_t>(SA, n, (w0 + tid) * FM_MROWS, s);
                    if (blk < n_blocks) occ[blk * G::BW + G::MW0 + tid % G::MWN] = m;
                }
                tc[tid] = (uint32_t)__builtin_popcount(m);
            }
            SYNC();
            PAR(tid) {
                if (tid == 0) {
                    uint32_t sum = run[0];
                    for (uint32_t b = 0; b < BPR; ++b) {
                        bc[b] = sum;
                        for (uint32_t i = 0; i < G::MWN; ++i) sum += tc[b * G::MWN + i];
                    }
                    run[0] = sum;
                }
            }
            SYNC();
            PAR(tid) {
                const uint64_t blk = (w0 + tid) / G::MWN;
                if (tid % G::MWN == 0 && blk < n_blocks) mrank[blk] = (idx_t)bc[tid / G::MWN];
            }
            SYNC();
        }
        PAR(tid) { if (tid == 0) cnt[4 * n_tiles + tile] = run[0]; }
        SYNC();
    }
}

// sample compaction in row order: the marked rows' SA values to samples[pre[tile] + mrank[block] + marks below in the block], and
// mrank[block] made absolute.  An index at or beyond cap (an SA that is no permutation marks too many rows) is not written.
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) fm_sample_kernel(KCTX const idx_t* __restrict__ SA, uint64_t n, uint64_t n_tiles, uint64_t n_blocks, uint32_t s,
                                                 const uint32_t* __restrict__ occ, idx_t* __restrict__ mrank, const uint64_t* __restrict__ pre,
                                                 idx_t* __restrict__ samples, uint64_t cap)
{
    using G = FmGeom<idx_t>;
    TL_DECL(uint64_t, at, 1);
    for (uint64_t tile = K_BLOCK_IDX; tile < n_tiles; tile += K_GRID_DIM) {         // block-uniform
        const uint64_t base = pre[4 * n_tiles + tile];
        for (uint32_t j = 0; j < FM_MROUNDS; ++j) {
            const uint64_t w0 = (tile * FM_MROUNDS + j) * FM_NT;
            PAR(tid) {
                const uint64_t blk = (w0 + tid) / G::MWN;
                uint64_t a = ~0ull;
                if (blk < n_blocks) {
                    a = base + (uint64_t)mrank[blk];
                    for (uint32_t i = 0; i < tid % G::MWN; ++i) a += (uint32_t)__builtin_popcount(occ[blk * G::BW + G::MW0 + i]);
                }
                TL(at, tid, 0) = a;
            }
            SYNC();
            PAR(tid) {
                const uint64_t blk = (w0 + tid) / G::MWN, r0 = (w0 + tid) * FM_MROWS;
                if (blk < n_blocks) {
                    uint64_t a = TL(at, tid, 0);
                    uint32_t m = occ[blk * G::BW + G::MW0 + tid % G::MWN];
                    while (m) {
                        const uint32_t b = (uint32_t)__builtin_ctz(m);
                        m &= m - 1;
                        const uint64_t r = r0 + b;
                        if (a < cap && r >= 1 && r <= n) samples[a] = SA[r - 1];
                        ++a;
                    }
                    if (tid % G::MWN == 0) mrank[blk] = (idx_t)(base + (uint64_t)mrank[blk]);
                }
            }
            SYNC();
        }
    }
}

// Occ(c, r) + the '$' correction from the block p of row r; k = r mod ROWS.  The count is read at its (dynamic) place, the code words
// at fixed offsets: one line, no indexed register array.
template <typename idx_t>
HD uint64_t fm_block_occ(const uint32_t* __restrict__ p, uint32_t c, uint32_t k, bool past_dollar)
{
    using G = FmGeom<idx_t>;
    uint64_t cnt = (uint64_t)reinterpret_cast<const idx_t*>(p)[c];
    uint32_t w[G::CWN];
    UNROLL
    for (uint32_t i = 0; i < G::CWN; ++i) w[i] = p[G::CW0 + i];
    UNROLL
    for (uint32_t i = 0; i < G::CWN; ++i) {
        const uint32_t rows = k > i * FM_WROWS ? (k - i * FM_WROWS < FM_WROWS ? k - i * FM_WROWS : FM_WROWS) : 0u;
        cnt += fm_word_rank(w[i], c, rows);
    }
    if (c == 0 && past_dollar) --cnt;
    return cnt;
}
// C[c] by selects (c differs from lane to lane: no indexed read of the kernel's arguments)
HD uint64_t fm_c_of(const FmView& v, uint32_t c) { return c == 0 ? v.C[0] : c == 1 ? v.C[1] : c == 2 ? v.C[2] : v.C[3]; }
// the block of row r, inside the Occ section whatever r is
template <typename idx_t>
HD const uint32_t* fm_block_of(const FmView& v, uint64_t r)
{
    using G = FmGeom<idx_t>;
    uint64_t b = r / G::ROWS;
    if (b >= v.n_blocks) b = v.n_blocks - 1;      // (never for r <= n + 1: n_blocks = (n + 1) / ROWS + 1)
    return v.occ + b * G::BW;
}
// row r (<= n + 1) -> C[c] + Occ(c, r), kept inside 0 .. n + 1
template <typename idx_t>
HD uint64_t fm_lf(const FmView& v, uint32_t c, uint64_t r)
{
    using G = FmGeom<idx_t>;
    const uint64_t x = fm_c_of(v, c) + fm_block_occ<idx_t>(fm_block_of<idx_t>(v, r), c, (uint32_t)(r % G::ROWS), r > v.primary + 1);
    return x <= v.n + 1 ? x : v.n + 1;
}

// count: one lane per pattern, backward search from the last byte; first[j] = the SA rank of the first occurrence, count[j]
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) fm_count_kernel(KCTX FmView v, const uint8_t* __restrict__ pat, const uint64_t* __restrict__ patoff, uint64_t q,
                                                uint64_t* __restrict__ first, uint64_t* __restrict__ count)
{
    const uint64_t stride = (uint64_t)K_GRID_DIM * FM_NT;
    for (uint64_t j0 = (uint64_t)K_BLOCK_IDX * FM_NT; j0 < q; j0 += stride) {       // block-uniform
        PAR(tid) {
            const uint64_t j = j0 + tid;
            if (j < q) {
                const uint64_t a = patoff[j], b = patoff[j + 1], m = b > a ? b - a : 0;
                uint64_t lo = m ? 0 : 1, hi = v.n + 1;                             // every row; without the '$' row for the empty pattern
                if (m > v.n) hi = lo;
                for (uint64_t i = m; i > 0 && lo < hi; --i) {
                    const uint32_t byte = pat[a + i - 1], c = fm_code_of(v.syms, v.sigma, byte);
                    if (!fm_is_letter(v.syms, v.sigma, byte, c)) { hi = lo; break; }
                    const uint64_t l2 = fm_lf<idx_t>(v, c, lo), h2 = fm_lf<idx_t>(v, c, hi);     // (independent: issued together)
                    lo = l2;
                    hi = h2;
                }
                first[j] = lo < hi ? lo - 1 : 0;
                count[j] = lo < hi ? hi - lo : 0;
            }
        }
    }
}

// entry checks of the query calls on the caller's device arrays: off[0 .. q] monotone (flag 1), first + count <= n (flag 2)
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) fm_check_kernel(KCTX const uint64_t* __restrict__ off, uint64_t q, const uint64_t* __restrict__ first,
                                                const uint64_t* __restrict__ count, uint64_t n, uint32_t* __restrict__ flags)
{
    const uint64_t stride = (uint64_t)K_GRID_DIM * FM_NT;
    for (uint64_t j0 = (uint64_t)K_BLOCK_IDX * FM_NT; j0 < q; j0 += stride) {       // block-uniform
        PAR(tid) {
            const uint64_t j = j0 + tid;
            if (j < q) {
                uint32_t f = off[j + 1] < off[j] ? 1u : 0u;
                if (first && (first[j] > n || count[j] > n - first[j])) f |= 2u;
                if (f) ATOMIC_OR_U32(flags, f);
            }
        }
    }
}

// locate: one lane per output position o in [off[0], off[q]): its query j by bisection over off, rank first[j] + t; LF steps to a
// marked row or the '$' row, at most s of them.  flags: 4 = a walk did not end (or met a sample index outside the samples).
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) fm_locate_kernel(KCTX FmView v, const uint64_t* __restrict__ first, const uint64_t* __restrict__ count,
                                                 const uint64_t* __restrict__ off, uint64_t q, uint64_t o_begin, uint64_t o_end,
                                                 uint64_t* __restrict__ pos, uint32_t* __restrict__ flags)
{
    using G = FmGeom<idx_t>;
    const uint64_t stride = (uint64_t)K_GRID_DIM * FM_NT;
    for (uint64_t o0 = o_begin + (uint64_t)K_BLOCK_IDX * FM_NT; o0 < o_end; o0 += stride) {     // block-uniform
        PAR(tid) {
            const uint64_t o = o0 + tid;
            if (o < o_end) {
                uint64_t a = 0, b = q;                                              // the last j with off[j] <= o
                while (b - a > 1) { const uint64_t mid = a + (b - a) / 2; if (off[mid] <= o) a = mid; else b = mid; }
                const uint64_t t = o - off[a];
                if (off[a] <= o && t < count[a] && first[a] + t < v.n) {
                    uint64_t r = first[a] + t + 1, res = ~0ull;
                    bool done = false;
                    for (uint32_t steps = 0; steps <= v.s; ++steps) {
                        if (r == v.primary + 1) { res = steps; done = true; break; }
                        const uint32_t* p = fm_block_of<idx_t>(v, r);
                        const uint32_t k = (uint32_t)(r % G::ROWS);
                        uint32_t mw[G::MWN];
                        UNROLL
                        for (uint32_t i = 0; i < G::MWN; ++i) mw[i] = p[G::MW0 + i];
                        const uint32_t cw = p[G::CW0 + k / FM_WROWS];
                        uint32_t below = 0, marked = 0;                             // marks below row k in the block; row k's own
                        UNROLL
                        for (uint32_t i = 0; i < G::MWN; ++i) {
                            const uint32_t rows = k > 32 * i ? (k - 32 * i < 32 ? k - 32 * i : 32) : 0u;
                            below += (uint32_t)__builtin_popcount(rows < 32 ? mw[i] & ((1u << rows) - 1u) : mw[i]);
                            if (k / 32 == i) marked = (mw[i] >> (k % 32)) & 1u;
                        }
                        if (marked) {
                            const uint64_t blk = r / G::ROWS;
                            const uint64_t si = (uint64_t)static_cast<const idx_t*>(v.mrank)[blk < v.n_blocks ? blk : v.n_blocks - 1] + below;
                            if (si < v.n_samples) { res = (uint64_t)static_cast<const idx_t*>(v.samples)[si] + steps; done = true; }
                            break;
                        }
                        const uint32_t c = (cw >> (2u * (k % FM_WROWS))) & 3u;
                        const uint64_t x = fm_c_of(v, c) + fm_block_occ<idx_t>(p, c, k, r > v.primary + 1);
                        r = x <= v.n ? (x ? x : 1) : v.n;                            // (a row of the index: 1 .. n)
                    }
                    if (!done) { ATOMIC_OR_U32(flags, 4u); res = (uint64_t)(idx_t)~(idx_t)0; }
                    pos[o] = res;
                }
            }
        }
    }
}

// ---- matching statistics and maximal exact matches (capi_impl.h fm_match_* / fm_mems_*; include/caps_sa_hip.h "FM-index: matching
// statistics") ------------------------------------------------------------------------------------------------------------------
// For end e of pattern P (1 <= e <= m): L[e] = the longest l <= e (<= max_len when max_len > 0) such that P[e - l .. e) occurs in
// the text, and its SA interval.  Nothing but the Occ blocks, C[] and the '$' row rule is read: an index without samples answers.

// one lane per (pattern, end): slot o in [o_begin, o_end) = [patoff[0], patoff[q]), its pattern j by bisection over patoff (the
// locate kernel's over off), e = o - patoff[j] + 1.  The count kernel's loop from byte e - 1 leftwards; the last non-empty (lo, hi)
// is kept, and the walk ends at an empty interval, a byte that is no letter, the pattern's first byte or after max_len steps: at
// most min(e, max_len) steps whatever the body holds.  len is written always, first / count when they are not null.
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) fm_match_kernel(KCTX FmView v, const uint8_t* __restrict__ pat, const uint64_t* __restrict__ patoff, uint64_t q,
                                                uint64_t o_begin, uint64_t o_end, uint32_t max_len, uint32_t* __restrict__ len,
                                                uint64_t* __restrict__ first, uint64_t* __restrict__ count)
{
    const uint64_t stride = (uint64_t)K_GRID_DIM * FM_NT;
    for (uint64_t o0 = o_begin + (uint64_t)K_BLOCK_IDX * FM_NT; o0 < o_end; o0 += stride) {     // block-uniform
        PAR(tid) {
            const uint64_t o = o0 + tid;
            if (o < o_end) {
                uint64_t a = 0, b = q;                                              // the last j with patoff[j] <= o
                while (b - a > 1) { const uint64_t mid = a + (b - a) / 2; if (patoff[mid] <= o) a = mid; else b = mid; }
                const uint64_t p0 = patoff[a];
                uint64_t steps = p0 <= o ? o - p0 + 1 : 0;                          // e: the bytes at and left of o in its pattern
                if (max_len && steps > max_len) steps = max_len;
                uint64_t lo = 0, hi = v.n + 1;
                uint32_t l = 0;
                for (uint64_t i = 0; i < steps; ++i) {
                    const uint32_t byte = pat[o - i], c = fm_code_of(v.syms, v.sigma, byte);
                    if (!fm_is_letter(v.syms, v.sigma, byte, c)) break;
                    const uint64_t l2 = fm_lf<idx_t>(v, c, lo), h2 = fm_lf<idx_t>(v, c, hi);     // (independent: issued together)
                    if (l2 >= h2) break;
                    lo = l2;
                    hi = h2;
                    ++l;
                }
                const bool hit = l != 0 && lo != 0;                                 // (lo >= C[0] = 1 after a step)
                len[o - o_begin] = hit ? l : 0u;
                if (first) first[o - o_begin] = hit ? lo - 1 : 0;
                if (count) count[o - o_begin] = hit ? hi - lo : 0;
            }
        }
    }
}

// a pattern longer than limit bytes: flag 16 (a MEM's start and length are 32-bit fields, len[] is u32)
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) fm_patlen_check_kernel(KCTX const uint64_t* __restrict__ off, uint64_t q, uint64_t limit, uint32_t* __restrict__ flags)
{
    const uint64_t stride = (uint64_t)K_GRID_DIM * FM_NT;
    for (uint64_t j0 = (uint64_t)K_BLOCK_IDX * FM_NT; j0 < q; j0 += stride) {       // block-uniform
        PAR(tid) {
            const uint64_t j = j0 + tid;
            if (j < q && off[j + 1] > off[j] && off[j + 1] - off[j] > limit) ATOMIC_OR_U32(flags, 16u);
        }
    }
}

// the MEM rule, one lane per slot t in [0, total]: the match ending at e is a MEM of at least min_len bytes iff L[e] >= min_len and
// it cannot be extended to the right: e = m, or L[e + 1] <= L[e] (a byte P[e] that is no letter gives L[e + 1] = 0, so the rule
// covers it).  It is left-maximal by construction.  flag[total .. padded) = 0.  The flags are scanned by fm_scan_kernel as columns
// of `per` slots, one workgroup each, and the columns' totals once more: the record slot of t is slot[t] + colbase[t / per].
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) fm_mem_flag_kernel(KCTX const uint32_t* __restrict__ len, const uint64_t* __restrict__ patoff, uint64_t q,
                                                   uint64_t total, uint64_t padded, uint32_t min_len, uint64_t* __restrict__ flag)
{
    const uint64_t stride = (uint64_t)K_GRID_DIM * FM_NT, o_begin = patoff[0];
    for (uint64_t t0 = (uint64_t)K_BLOCK_IDX * FM_NT; t0 < padded; t0 += stride) {  // block-uniform
        PAR(tid) {
            const uint64_t t = t0 + tid;
            if (t < total) {
                const uint64_t o = o_begin + t;
                uint64_t a = 0, b = q;                                              // the last j with patoff[j] <= o
                while (b - a > 1) { const uint64_t mid = a + (b - a) / 2; if (patoff[mid] <= o) a = mid; else b = mid; }
                const uint32_t l = len[t];
                const bool last = o + 1 >= patoff[a + 1];                           // e = m
                flag[t] = l >= min_len && (last || len[t + 1] <= l) ? 1u : 0u;
            } else if (t < padded) {
                flag[t] = 0;
            }
        }
    }
}

// memoff[j] = the MEMs of the patterns before j: the scanned flags at pattern j's first slot (memoff[q] = all of them)
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) fm_mem_off_kernel(KCTX const uint64_t* __restrict__ slot, const uint64_t* __restrict__ colbase, uint64_t per,
                                                  const uint64_t* __restrict__ patoff, uint64_t q, uint64_t total, uint64_t* __restrict__ memoff)
{
    const uint64_t stride = (uint64_t)K_GRID_DIM * FM_NT, o_begin = patoff[0];
    for (uint64_t j0 = (uint64_t)K_BLOCK_IDX * FM_NT; j0 <= q; j0 += stride) {      // block-uniform
        PAR(tid) {
            const uint64_t j = j0 + tid;
            if (j <= q) {
                const uint64_t t = std::min<uint64_t>(patoff[j] >= o_begin ? patoff[j] - o_begin : 0, total);
                memoff[j] = slot[t] + colbase[t / per];
            }
        }
    }
}

// the records, 4 words of 64 bits each: pattern | start + (length << 32) | first | count, at the slot the scan gave: (pattern,
// increasing end) order.  A slot is a MEM's when the scan moves on behind it; one at or beyond cap is not written.
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) fm_mem_write_kernel(KCTX const uint32_t* __restrict__ len, const uint64_t* __restrict__ first,
                                                    const uint64_t* __restrict__ count, const uint64_t* __restrict__ slot,
                                                    const uint64_t* __restrict__ colbase, uint64_t per,
                                                    const uint64_t* __restrict__ patoff, uint64_t q, uint64_t total, uint64_t cap,
                                                    uint64_t* __restrict__ mems)
{
    const uint64_t stride = (uint64_t)K_GRID_DIM * FM_NT, o_begin = patoff[0];
    for (uint64_t t0 = (uint64_t)K_BLOCK_IDX * FM_NT; t0 < total; t0 += stride) {   // block-uniform
        PAR(tid) {
            const uint64_t t = t0 + tid;
            if (t < total) {
                const uint64_t at = slot[t] + colbase[t / per];
                if (slot[t + 1] + colbase[(t + 1) / per] != at && at < cap) {
                    const uint64_t o = o_begin + t;
                    uint64_t a = 0, b = q;                                          // the last j with patoff[j] <= o
                    while (b - a > 1) { const uint64_t mid = a + (b - a) / 2; if (patoff[mid] <= o) a = mid; else b = mid; }
                    const uint64_t e = o - patoff[a] + 1, l = len[t];
                    mems[4 * at] = a;
                    mems[4 * at + 1] = ((e - l) & 0xFFFFFFFFull) | (l << 32);
                    mems[4 * at + 2] = first[t];
                    mems[4 * at + 3] = count[t];
                }
            }
        }
    }
}

// ---- wide FM-index: 1 .. 256 letters (capi_impl.h fmw_*; include/caps_sa_hip.h "FM-index: the wide format") -------------------------
// A 4-ary wavelet matrix over the letter codes, every level an Occ section of the blocks above.  A code has Lv base-4 digits, digit 0
// the most significant; level 0 is the code sequence in row order ('$' row and the rows behind n: code 0), level l + 1 is level l
// stably partitioned by its level-l digit.  With Z[l][d] = the rows of level l with a digit below d and zone[c] = where code c gets
// from position 0:   p = r;  for l < Lv: d = digit_l(c), p = Z[l][d] + Occ_l(d, p);   LF(c, r) = C[c] + p - zone[c] - ['$' below r]
// -- one line per level, the narrow step exactly when Lv = 1.  The table section (letters, code_of, C, zone, Z: FMW_TAB_BYTES from
// FmwView::tab, checked on the host) is copied to LDS by every query workgroup; lanes index LDS, never a register array.  Every
// position is kept inside 0 .. n + 1 and every block inside its level at every level, whatever the tables and the body hold.
constexpr uint32_t FMW_MAX_LV = 4;
constexpr uint32_t FMW_TAB_LETTERS = 0, FMW_TAB_CODE = 256, FMW_TAB_C = 512, FMW_TAB_ZONE = FMW_TAB_C + 257 * 8,
                   FMW_TAB_Z = FMW_TAB_ZONE + 256 * 8, FMW_TAB_USED = FMW_TAB_Z + 4 * FMW_MAX_LV * 8;     // 4,744 bytes
constexpr uint32_t FMW_TAB_WORDS = FMW_TAB_USED / 8;          // 593 words of 64 bits
constexpr uint32_t FMW_TAB_BYTES = (FMW_TAB_USED + 63) / 64 * 64;                                         // 4,800 in the blob
struct FmwView {
    uint64_t n, primary;
    uint64_t n_blocks, n_samples;
    uint64_t lev_words;                        // 32-bit words of one level section
    const uint32_t* lev0;                      // level l at lev0 + l * lev_words
    const void* mrank;
    const void* samples;
    const uint64_t* tab;                       // the table section (device memory)
    uint32_t sigma, Lv, s;                     // Lv = 0: not a wide blob
};
// views into the LDS copy of the table section
HD const uint8_t* fmw_letters(const uint64_t* t) { return reinterpret_cast<const uint8_t*>(t) + FMW_TAB_LETTERS; }
HD const uint8_t* fmw_codes(const uint64_t* t) { return reinterpret_cast<const uint8_t*>(t) + FMW_TAB_CODE; }
HD const uint64_t* fmw_C(const uint64_t* t) { return t + FMW_TAB_C / 8; }
HD const uint64_t* fmw_zone(const uint64_t* t) { return t + FMW_TAB_ZONE / 8; }
HD const uint64_t* fmw_Z(const uint64_t* t) { return t + FMW_TAB_Z / 8; }
#define FMW_LOAD_TABLE(tab, w)                                                                    \
    SHARED_ARRAY(uint64_t, tab, FMW_TAB_WORDS);                                                   \
    PAR(tid) { for (uint32_t k = tid; k < FMW_TAB_WORDS; k += FM_NT) tab[k] = (w).tab[k]; }       \
    SYNC()

// the block of position p of level l, inside the level whatever p is
template <typename idx_t>
HD const uint32_t* fmw_block_of(const FmwView& w, uint32_t l, uint64_t p)
{
    using G = FmGeom<idx_t>;
    uint64_t b = p / G::ROWS;
    if (b >= w.n_blocks) b = w.n_blocks - 1;
    return w.lev0 + (uint64_t)l * w.lev_words + b * G::BW;
}
// the end of an LF step: position p of the last level -> the row, inside 0 .. n + 1
HD uint64_t fmw_row(const FmwView& w, const uint64_t* tab, uint32_t c, uint64_t p, bool past_dollar)
{
    const uint64_t z = fmw_zone(tab)[c];
    uint64_t k = p > z ? p - z : 0;
    if (c == 0 && past_dollar && k) --k;
    const uint64_t x = fmw_C(tab)[c] + k;
    return x <= w.n + 1 ? x : w.n + 1;
}
// LF(c, lo) and LF(c, hi): both positions go down together, their two lines of a level are issued together
template <typename idx_t>
HD void fmw_lf2(const FmwView& w, const uint64_t* tab, uint32_t c, uint64_t& lo, uint64_t& hi)
{
    using G = FmGeom<idx_t>;
    uint64_t pl = lo, ph = hi;
    for (uint32_t l = 0; l < w.Lv; ++l) {
        const uint32_t d = (c >> (2u * (w.Lv - 1u - l))) & 3u;
        const uint64_t z = fmw_Z(tab)[4 * l + d];
        const uint64_t a = fm_block_occ<idx_t>(fmw_block_of<idx_t>(w, l, pl), d, (uint32_t)(pl % G::ROWS), false);
        const uint64_t b = fm_block_occ<idx_t>(fmw_block_of<idx_t>(w, l, ph), d, (uint32_t)(ph % G::ROWS), false);
        pl = z + a <= w.n + 1 ? z + a : w.n + 1;
        ph = z + b <= w.n + 1 ? z + b : w.n + 1;
    }
    lo = fmw_row(w, tab, c, pl, lo > w.primary + 1);
    hi = fmw_row(w, tab, c, ph, hi > w.primary + 1);
}

// ---- the build ----
// the codes of rows 0 .. n in row order (level 0), one byte each ('$' row: 0; the bytes up to the next multiple of 16: 0), and the
// rows of every code: hist[code * K_GRID_DIM + workgroup] (fm_scan_kernel sums the columns).  code_of: the table in device memory.
// The histogram has 8 copies in LDS, one per lane mod 8: with a few letters every lane of a wave would hit the same few words.
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) fmw_code_kernel(KCTX const uint8_t* __restrict__ B, uint64_t n, uint64_t primary, const uint8_t* __restrict__ code_of,
                                                uint8_t* __restrict__ codes, uint64_t* __restrict__ hist)
{
    static_assert(FM_NT == 256, "one thread per entry of lut[] and of every histogram copy");
    SHARED_ARRAY(uint32_t, lut, 256);
    SHARED_ARRAY(uint32_t, h, 8 * 256);
    PAR(tid) {
        lut[tid] = code_of[tid];
        for (uint32_t k = 0; k < 8; ++k) h[k * 256 + tid] = 0;
    }
    SYNC();
    const uint64_t chunks = n / FM_WROWS + 1, stride = (uint64_t)K_GRID_DIM * FM_NT;         // rows 0 .. n
    for (uint64_t c0 = (uint64_t)K_BLOCK_IDX * FM_NT; c0 < chunks; c0 += stride) {           // block-uniform
        PAR(tid) {
            const uint64_t ch = c0 + tid;
            if (ch < chunks) {
                const uint64_t r0 = ch * FM_WROWS;
                uint32_t out[4] = {0, 0, 0, 0};
                uint32_t* hh = h + (tid & 7u) * 256;
                if (r0 >= FM_WROWS && r0 + FM_WROWS <= n && !(primary + 1 >= r0 && primary + 1 < r0 + FM_WROWS)) {
                    uint32_t x[4];
                    UNROLL
                    for (uint32_t k = 0; k < 4; ++k) x[k] = STREAM_LOAD(reinterpret_cast<const u32_any_align*>(B + r0) + k);
                    uint32_t prev = B[r0 - 1];
                    UNROLL
                    for (uint32_t j = 0; j < FM_WROWS; ++j) {
                        const uint32_t c = lut[prev];
                        out[j / 4] |= c << (8u * (j % 4));
                        FETCH_ADD_U32(&hh[c], 1u);
                        prev = (x[j / 4] >> (8u * (j % 4))) & 0xFFu;
                    }
                } else {
                    for (uint32_t j = 0; j < FM_WROWS; ++j) {
                        const uint64_t r = r0 + j;
                        if (r > n) continue;
                        const uint32_t c = r == primary + 1 ? 0u : lut[B[r ? r - 1 : primary]];
                        out[j / 4] |= c << (8u * (j % 4));
                        FETCH_ADD_U32(&hh[c], 1u);
                    }
                }
                UNROLL
                for (uint32_t k = 0; k < 4; ++k) reinterpret_cast<uint32_t*>(codes + r0)[k] = out[k];
            }
        }
    }
    SYNC();
    PAR(tid) {
        uint64_t s = 0;
        for (uint32_t k = 0; k < 8; ++k) s += h[k * 256 + tid];
        hist[(uint64_t)tid * K_GRID_DIM + K_BLOCK_IDX] = s;
    }
}

// the digit word of rows r0 .. r0 + 15 of a level (r0 a multiple of 16): digit = (code >> shift) & 3; rows behind n: 0
HD uint32_t fmw_digit_word(const uint8_t* __restrict__ codes, uint64_t n, uint64_t r0, uint32_t shift)
{
    uint32_t w = 0;
    if (r0 + FM_WROWS <= n + 1) {
        uint32_t x[4];
        UNROLL
        for (uint32_t k = 0; k < 4; ++k) x[k] = reinterpret_cast<const uint32_t*>(codes + r0)[k];
        UNROLL
        for (uint32_t j = 0; j < FM_WROWS; ++j) w |= (((x[j / 4] >> (8u * (j % 4))) >> shift) & 3u) << (2u * j);
    } else {
        for (uint32_t j = 0; j < FM_WROWS; ++j)
            if (r0 + j <= n) w |= (((uint32_t)codes[r0 + j] >> shift) & 3u) << (2u * j);
    }
    return w;
}

// fm_tile_count_kernel on a level's codes: per tile the rows of each digit -> cnt[digit * n_tiles + tile]
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) fmw_count_kernel(KCTX const uint8_t* __restrict__ codes, uint64_t n, uint64_t n_tiles, uint32_t shift,
                                                 uint64_t* __restrict__ cnt)
{
    SHARED_ARRAY(uint32_t, h, 4);
    for (uint64_t tile = K_BLOCK_IDX; tile < n_tiles; tile += K_GRID_DIM) {         // block-uniform
        PAR(tid) { if (tid < 4) h[tid] = 0; }
        SYNC();
        PAR(tid) {
            uint32_t c[4] = {0, 0, 0, 0};
            for (uint32_t j = 0; j < FM_ROUNDS; ++j) {
                const uint64_t r0 = tile * FM_TILE + ((uint64_t)j * FM_NT + tid) * FM_WROWS;
                const uint32_t w = fmw_digit_word(codes, n, r0, shift);
                UNROLL
                for (uint32_t k = 0; k < 4; ++k) c[k] += fm_word_rank(w, k, FM_WROWS);
            }
            for (uint32_t k = 0; k < 4; ++k) if (c[k]) FETCH_ADD_U32(&h[k], c[k]);
        }
        SYNC();
        PAR(tid) { if (tid < 4) cnt[(uint64_t)tid * n_tiles + tile] = h[tid]; }
        SYNC();
    }
}

// fm_pack_kernel on a level's codes: the blocks of the level, mark words zero
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) fmw_pack_kernel(KCTX const uint8_t* __restrict__ codes, uint64_t n, uint64_t n_tiles, uint64_t n_blocks, uint32_t shift,
                                                const uint64_t* __restrict__ pre, uint32_t* __restrict__ occ)
{
    using G = FmGeom<idx_t>;
    constexpr uint32_t BPR = FM_NT / G::CWN;      // blocks of a round
    SHARED_ARRAY(uint32_t, tc, 4 * FM_NT);        // [digit][thread]
    SHARED_ARRAY(uint64_t, bc, 4 * BPR);          // [digit][block of the round]: the sum, then the absolute count before the block
    SHARED_ARRAY(uint64_t, run, 4);
    TL_DECL(uint32_t, wd, 1);
    for (uint64_t tile = K_BLOCK_IDX; tile < n_tiles; tile += K_GRID_DIM) {         // block-uniform
        PAR(tid) { if (tid < 4) run[tid] = pre[(uint64_t)tid * n_tiles + tile]; }
        SYNC();
        for (uint32_t j = 0; j < FM_ROUNDS; ++j) {
            const uint64_t w0 = (tile * FM_ROUNDS + j) * FM_NT;                     // first digit word of the round
            PAR(tid) {
                const uint32_t w = fmw_digit_word(codes, n, (w0 + tid) * FM_WROWS, shift);
                TL(wd, tid, 0) = w;
                UNROLL
                for (uint32_t k = 0; k < 4; ++k) tc[k * FM_NT + tid] = fm_word_rank(w, k, FM_WROWS);
            }
            SYNC();
            PAR(tid) {
                if (tid % G::CWN == 0) {
                    for (uint32_t k = 0; k < 4; ++k) {
                        uint32_t s = 0;
                        for (uint32_t i = 0; i < G::CWN; ++i) s += tc[k * FM_NT + tid + i];
                        bc[k * BPR + tid / G::CWN] = s;
                    }
                }
            }
            SYNC();
            PAR(tid) {
                if (tid < 4) {
                    uint64_t s = run[tid];
                    for (uint32_t i = 0; i < BPR; ++i) { const uint64_t v = bc[tid * BPR + i]; bc[tid * BPR + i] = s; s += v; }
                    run[tid] = s;
                }
            }
            SYNC();
            PAR(tid) {
                const uint64_t blk = (w0 + tid) / G::CWN;
                if (blk < n_blocks) {
                    uint32_t* p = occ + blk * G::BW;
                    p[G::CW0 + tid % G::CWN] = TL(wd, tid, 0);
                    if (tid % G::CWN == 0) {
                        for (uint32_t k = 0; k < 4; ++k) reinterpret_cast<idx_t*>(p)[k] = (idx_t)bc[k * BPR + tid / G::CWN];
                        for (uint32_t k = 0; k < G::MWN; ++k) p[G::MW0 + k] = 0;
                    }
                }
            }
            SYNC();
        }
    }
}

// the stable partition of a level by its digit: row r of digit d goes to  zd + pre[d][tile] + (rows of digit d before r in the tile),
// zd = the rows of the level with a digit below d.  A thread owns FMW_SROWS consecutive rows; the threads' 4 counts, 16 bits each in one
// word (a tile has 16,384 rows), are scanned over the workgroup; the tile is laid out in LDS digit by digit and leaves as 4 contiguous
// runs: aligned words, single bytes only at a run's two ends.  Rows behind n are neither counted nor moved.  cap: the bytes of `out`.
constexpr uint32_t FMW_SROWS = (uint32_t)(FM_TILE / FM_NT);   // 64
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) fmw_scatter_kernel(KCTX const uint8_t* __restrict__ codes, uint8_t* __restrict__ out, uint64_t n, uint64_t cap,
                                                   uint64_t n_tiles, uint32_t shift, const uint64_t* __restrict__ pre, uint64_t z1, uint64_t z2,
                                                   uint64_t z3)
{
    SHARED_ARRAY(uint64_t, sa, FM_NT);
    SHARED_ARRAY(uint64_t, sb, FM_NT);
    SHARED_ARRAY(uint8_t, stage, FM_TILE);
    TL_DECL(uint32_t, cw, FMW_SROWS / 4);
    TL_DECL(uint64_t, own, 1);
    for (uint64_t tile = K_BLOCK_IDX; tile < n_tiles; tile += K_GRID_DIM) {         // block-uniform
        PAR(tid) {
            const uint64_t r0 = tile * FM_TILE + (uint64_t)tid * FMW_SROWS;
            const uint32_t rows = r0 > n ? 0u : (uint32_t)std::min<uint64_t>(FMW_SROWS, n + 1 - r0);
            uint64_t c = 0;
            for (uint32_t k = 0; k < FMW_SROWS / 4; ++k) {
                uint32_t x = 0;
                if (4 * k < rows) x = reinterpret_cast<const uint32_t*>(codes + r0)[k];           // (the buffer ends at a multiple of 64)
                TL(cw, tid, k) = x;
                for (uint32_t j = 0; j < 4; ++j)
                    if (4 * k + j < rows) c += 1ull << (16u * (((x >> (8u * j)) >> shift) & 3u));
            }
            TL(own, tid, 0) = c;
            sa[tid] = c;
        }
        SYNC();
        // inclusive scan over the threads, ping-pong between sa and sb: after the 8 steps the result is in sa again
        for (uint32_t d = 1; d < FM_NT; d *= 4) {
            PAR(tid) { sb[tid] = sa[tid] + (tid >= d ? sa[tid - d] : 0); }
            SYNC();
            PAR(tid) { sa[tid] = sb[tid] + (tid >= 2 * d ? sb[tid - 2 * d] : 0); }
            SYNC();
        }
        PAR(tid) {
            const uint64_t tot = sa[FM_NT - 1], own = TL(own, tid, 0), ex = sa[tid] - own;
            uint32_t at[4];
            uint32_t base = 0;
            UNROLL
            for (uint32_t d = 0; d < 4; ++d) { at[d] = base + (uint32_t)((ex >> (16u * d)) & 0xFFFFu); base += (uint32_t)((tot >> (16u * d)) & 0xFFFFu); }
            const uint32_t rows = (uint32_t)(((own >> 0) & 0xFFFFu) + ((own >> 16) & 0xFFFFu) + ((own >> 32) & 0xFFFFu) + ((own >> 48) & 0xFFFFu));
            for (uint32_t k = 0; k < FMW_SROWS / 4; ++k) {
                const uint32_t x = TL(cw, tid, k);
                for (uint32_t j = 0; j < 4; ++j) {
                    if (4 * k + j >= rows) break;
                    const uint32_t b = (x >> (8u * j)) & 0xFFu, d = (b >> shift) & 3u;
                    // (no indexed register array: the cursor of digit d by selects)
                    const uint32_t p = d == 0 ? at[0] : d == 1 ? at[1] : d == 2 ? at[2] : at[3];
                    if (p < FM_TILE) stage[p] = (uint8_t)b;
                    at[0] += d == 0; at[1] += d == 1; at[2] += d == 2; at[3] += d == 3;
                }
            }
        }
        SYNC();
        PAR(tid) {
            const uint64_t tot = sa[FM_NT - 1];
            uint32_t s0 = 0;                                                         // the run's first byte in stage
            for (uint32_t d = 0; d < 4; ++d) {
                const uint32_t len = (uint32_t)((tot >> (16u * d)) & 0xFFFFu);
                const uint64_t D = (d == 0 ? 0 : d == 1 ? z1 : d == 2 ? z2 : z3) + pre[(uint64_t)d * n_tiles + tile];
                const uint32_t head = std::min<uint32_t>(len, (uint32_t)((4u - (D & 3u)) & 3u)), nw = (len - head) / 4, tail0 = head + 4 * nw;
                if (tid < head && D + tid < cap) out[D + tid] = stage[s0 + tid];
                for (uint32_t w = tid; w < nw; w += FM_NT) {
                    const uint32_t k = s0 + head + 4 * w;
                    const uint32_t v = (uint32_t)stage[k] | ((uint32_t)stage[k + 1] << 8) | ((uint32_t)stage[k + 2] << 16) | ((uint32_t)stage[k + 3] << 24);
                    if (D + head + 4ull * w + 4 <= cap) *reinterpret_cast<uint32_t*>(out + D + head + 4ull * w) = v;
                }
                if (tid < len - tail0 && D + tail0 + tid < cap) out[D + tail0 + tid] = stage[s0 + tail0 + tid];
                s0 += len;
            }
        }
        SYNC();
    }
}

// ---- the queries: the narrow kernels' loops, the LF step above ----
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) fmw_count_q_kernel(KCTX FmwView v, const uint8_t* __restrict__ pat, const uint64_t* __restrict__ patoff, uint64_t q,
                                                   uint64_t* __restrict__ first, uint64_t* __restrict__ count)
{
    FMW_LOAD_TABLE(tab, v);
    const uint64_t stride = (uint64_t)K_GRID_DIM * FM_NT;
    for (uint64_t j0 = (uint64_t)K_BLOCK_IDX * FM_NT; j0 < q; j0 += stride) {       // block-uniform
        PAR(tid) {
            const uint64_t j = j0 + tid;
            if (j < q) {
                const uint64_t a = patoff[j], b = patoff[j + 1], m = b > a ? b - a : 0;
                uint64_t lo = m ? 0 : 1, hi = v.n + 1;                             // every row; without the '$' row for the empty pattern
                if (m > v.n) hi = lo;
                for (uint64_t i = m; i > 0 && lo < hi; --i) {
                    const uint32_t byte = pat[a + i - 1], c = fmw_codes(tab)[byte];
                    if (!(c < v.sigma && fmw_letters(tab)[c] == byte)) { hi = lo; break; }
                    fmw_lf2<idx_t>(v, tab, c, lo, hi);
                }
                first[j] = lo < hi ? lo - 1 : 0;
                count[j] = lo < hi ? hi - lo : 0;
            }
        }
    }
}

// locate: fm_locate_kernel; the code of a row comes from the descent itself (the digit at the position instead of the pattern's)
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) fmw_locate_kernel(KCTX FmwView v, const uint64_t* __restrict__ first, const uint64_t* __restrict__ count,
                                                  const uint64_t* __restrict__ off, uint64_t q, uint64_t o_begin, uint64_t o_end,
                                                  uint64_t* __restrict__ pos, uint32_t* __restrict__ flags)
{
    using G = FmGeom<idx_t>;
    FMW_LOAD_TABLE(tab, v);
    const uint64_t stride = (uint64_t)K_GRID_DIM * FM_NT;
    for (uint64_t o0 = o_begin + (uint64_t)K_BLOCK_IDX * FM_NT; o0 < o_end; o0 += stride) {     // block-uniform
        PAR(tid) {
            const uint64_t o = o0 + tid;
            if (o < o_end) {
                uint64_t a = 0, b = q;                                              // the last j with off[j] <= o
                while (b - a > 1) { const uint64_t mid = a + (b - a) / 2; if (off[mid] <= o) a = mid; else b = mid; }
                const uint64_t t = o - off[a];
                if (off[a] <= o && t < count[a] && first[a] + t < v.n) {
                    uint64_t r = first[a] + t + 1, res = ~0ull;
                    bool done = false;
                    for (uint32_t steps = 0; steps <= v.s; ++steps) {
                        if (r == v.primary + 1) { res = steps; done = true; break; }
                        const uint32_t* p = fmw_block_of<idx_t>(v, 0, r);
                        uint32_t k = (uint32_t)(r % G::ROWS);
                        uint32_t mw[G::MWN];
                        UNROLL
                        for (uint32_t i = 0; i < G::MWN; ++i) mw[i] = p[G::MW0 + i];
                        uint32_t below = 0, marked = 0;                             // marks below row k in the block; row k's own
                        UNROLL
                        for (uint32_t i = 0; i < G::MWN; ++i) {
                            const uint32_t rows = k > 32 * i ? (k - 32 * i < 32 ? k - 32 * i : 32) : 0u;
                            below += (uint32_t)__builtin_popcount(rows < 32 ? mw[i] & ((1u << rows) - 1u) : mw[i]);
                            if (k / 32 == i) marked = (mw[i] >> (k % 32)) & 1u;
                        }
                        if (marked) {
                            const uint64_t blk = r / G::ROWS;
                            const uint64_t si = (uint64_t)static_cast<const idx_t*>(v.mrank)[blk < v.n_blocks ? blk : v.n_blocks - 1] + below;
                            if (si < v.n_samples) { res = (uint64_t)static_cast<const idx_t*>(v.samples)[si] + steps; done = true; }
                            break;
                        }
                        uint32_t c = 0;
                        uint64_t x = r;
                        for (uint32_t l = 0; l < v.Lv; ++l) {
                            if (l) { p = fmw_block_of<idx_t>(v, l, x); k = (uint32_t)(x % G::ROWS); }
                            const uint32_t d = (p[G::CW0 + k / FM_WROWS] >> (2u * (k % FM_WROWS))) & 3u;
                            c = 4 * c + d;
                            x = fmw_Z(tab)[4 * l + d] + fm_block_occ<idx_t>(p, d, k, false);
                            if (x > v.n + 1) x = v.n + 1;
                        }
                        x = fmw_row(v, tab, c, x, r > v.primary + 1);
                        r = x <= v.n ? (x ? x : 1) : v.n;                            // (a row of the index: 1 .. n)
                    }
                    if (!done) { ATOMIC_OR_U32(flags, 4u); res = (uint64_t)(idx_t)~(idx_t)0; }
                    pos[o] = res;
                }
            }
        }
    }
}

template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) fmw_match_kernel(KCTX FmwView v, const uint8_t* __restrict__ pat, const uint64_t* __restrict__ patoff, uint64_t q,
                                                 uint64_t o_begin, uint64_t o_end, uint32_t max_len, uint32_t* __restrict__ len,
                                                 uint64_t* __restrict__ first, uint64_t* __restrict__ count)
{
    FMW_LOAD_TABLE(tab, v);
    const uint64_t stride = (uint64_t)K_GRID_DIM * FM_NT;
    for (uint64_t o0 = o_begin + (uint64_t)K_BLOCK_IDX * FM_NT; o0 < o_end; o0 += stride) {     // block-uniform
        PAR(tid) {
            const uint64_t o = o0 + tid;
            if (o < o_end) {
                uint64_t a = 0, b = q;                                              // the last j with patoff[j] <= o
                while (b - a > 1) { const uint64_t mid = a + (b - a) / 2; if (patoff[mid] <= o) a = mid; else b = mid; }
                const uint64_t p0 = patoff[a];
                uint64_t steps = p0 <= o ? o - p0 + 1 : 0;                          // e: the bytes at and left of o in its pattern
                if (max_len && steps > max_len) steps = max_len;
                uint64_t lo = 0, hi = v.n + 1;
                uint32_t l = 0;
                for (uint64_t i = 0; i < steps; ++i) {
                    const uint32_t byte = pat[o - i], c = fmw_codes(tab)[byte];
                    if (!(c < v.sigma && fmw_letters(tab)[c] == byte)) break;
                    uint64_t l2 = lo, h2 = hi;
                    fmw_lf2<idx_t>(v, tab, c, l2, h2);
                    if (l2 >= h2) break;
                    lo = l2;
                    hi = h2;
                    ++l;
                }
                const bool hit = l != 0 && lo != 0;                                 // (lo >= C[0] = 1 after a step)
                len[o - o_begin] = hit ? l : 0u;
                if (first) first[o - o_begin] = hit ? lo - 1 : 0;
                if (count) count[o - o_begin] = hit ? hi - lo : 0;
            }
        }
    }
}

// ---- SA samples from the BWT alone (capi_impl.h fm_from_bwt_*; include/caps_sa_hip.h "FM-index from the BWT alone") -------------
// LF^k(0), k = 1 .. n, is the row of text position n - k (k = n: the '$' row, position 0; k = n + 1: row 0 again), so a row's offset
// on the cycle of row 0 is its SA value: neither T nor the SA is read.  LF comes from the finished Occ section, one block per step
// (the inverse BWT's 4-byte table load, ibwt_walk_kernel, replaced by one line); the splitters are the inverse's (every IBWT_S0-th
// row) and their list is ranked by its IBWT_LINK / ibwt_top_kernel / IBWT_PROP, which never touch LF.

// LF of row r (<= n) from its block: the '$' row goes to row 0; kept inside 0 .. n whatever the block holds
template <typename idx_t>
HD uint64_t fm_lf_row(const FmView& v, uint64_t r)
{
    using G = FmGeom<idx_t>;
    if (r == v.primary + 1) return 0;
    const uint32_t* p = fm_block_of<idx_t>(v, r);
    const uint32_t k = (uint32_t)(r % G::ROWS);
    const uint32_t c = (p[G::CW0 + k / FM_WROWS] >> (2u * (k % FM_WROWS))) & 3u;
    const uint64_t x = fm_c_of(v, c) + fm_block_occ<idx_t>(p, c, k, r > v.primary + 1);
    return x <= v.n ? x : v.n;
}

// The two walks over the Occ section, in ibwt_walk_kernel's ranges of IBWT_Q walks per workgroup:
//   FMW_LINK0  from splitter row j * S0 along LF to the next splitter: succ[j], len[j] (rows; at most n + 1 steps)
//   FMW_MARK   from splitter row j * S0 at cycle offset off[j] for len[j] rows: the row at offset k in 1 .. n has text position
//              p = n - k; when p is a multiple of s its mark bit is set (an atomic OR into the block's mark word: the lanes that
//              pass through the block meanwhile read its counts and code words only) and stage[p / s] = the row (each slot once).
//              Offset 0 is row 0, never marked; offset n is the '$' row (p = 0), marked.
enum { FMW_LINK0 = 0, FMW_MARK = 1 };
template <typename idx_t, int MODE>
GLOBAL_FN LAUNCH_BOUNDS(IBWT_NT) fm_walk_kernel(KCTX FmView v, uint64_t walks, idx_t* __restrict__ succ, uint64_t* __restrict__ len,
                                                 const uint64_t* __restrict__ off, uint32_t* occ, idx_t* __restrict__ stage)
{
    using G = FmGeom<idx_t>;
    SHARED_ARRAY(uint32_t, q, 1);
    const uint64_t ranges = (walks + IBWT_Q - 1) / IBWT_Q;
    const uint32_t sh = (uint32_t)__builtin_ctz(v.s | (FM_MAX_SAMPLE << 1));
    for (uint64_t rg = K_BLOCK_IDX; rg < ranges; rg += K_GRID_DIM) {               // block-uniform
        PAR(tid) { if (tid == 0) q[0] = 0; }
        SYNC();
        PAR(tid) {
            const uint64_t lo = rg * IBWT_Q, cnt = std::min<uint64_t>(IBWT_Q, walks - lo);
            for (;;) {
                const uint32_t i = FETCH_ADD_U32(&q[0], 1u);
                if (i >= cnt) break;
                const uint64_t j = lo + i;
                uint64_t cur = j << IBWT_S0_LOG;
                if (cur > v.n) continue;                                            // (never: walks = n / S0 + 1)
                if (MODE == FMW_LINK0) {
                    uint64_t steps = 0;
                    do { cur = fm_lf_row<idx_t>(v, cur); ++steps; } while ((cur & (IBWT_S0 - 1)) != 0 && steps <= v.n);
                    succ[j] = (idx_t)(cur >> IBWT_S0_LOG);
                    len[j] = steps;
                } else {
                    const uint64_t o = off[j], steps = std::min<uint64_t>(len[j], v.n + 1);
                    for (uint64_t t = 0; t < steps; ++t) {
                        const uint64_t k = o + t;
                        if (k > v.n || k < o) break;                                // (never, after the single-cycle check)
                        const uint64_t p = v.n - k;
                        if (k >= 1 && (p & (v.s - 1u)) == 0 && (p >> sh) < v.n_samples) {
                            ATOMIC_OR_U32(&occ[(cur / G::ROWS) * G::BW + G::MW0 + (uint32_t)(cur % G::ROWS) / FM_MROWS], 1u << (cur % FM_MROWS));
                            stage[p >> sh] = (idx_t)cur;
                        }
                        if (t + 1 < steps) cur = fm_lf_row<idx_t>(v, cur);
                    }
                }
            }
        }
        SYNC();
    }
}

// mrank[block] from tile-relative (fm_mark_kernel) to absolute: + the marks of the tiles before the block's (pre[4][tile], scanned)
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) fm_mrank_abs_kernel(KCTX idx_t* __restrict__ mrank, uint64_t n_blocks, uint64_t n_tiles,
                                                    const uint64_t* __restrict__ pre)
{
    using G = FmGeom<idx_t>;
    const uint64_t stride = (uint64_t)K_GRID_DIM * FM_NT;
    for (uint64_t b0 = (uint64_t)K_BLOCK_IDX * FM_NT; b0 < n_blocks; b0 += stride) { // block-uniform
        PAR(tid) {
            const uint64_t b = b0 + tid, tile = b * G::ROWS / FM_TILE;
            if (b < n_blocks && tile < n_tiles) mrank[b] = (idx_t)(pre[4 * n_tiles + tile] + (uint64_t)mrank[b]);
        }
    }
}

// the samples in row order from the staged rows: samples[mrank[block of stage[i]] + marks below the row in its block] = i * s.
// Every index is compared with its section's size before it is used (the query kernels' rule).
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) fm_place_kernel(KCTX FmView v, const idx_t* __restrict__ stage, idx_t* __restrict__ samples)
{
    using G = FmGeom<idx_t>;
    const uint64_t stride = (uint64_t)K_GRID_DIM * FM_NT;
    for (uint64_t i0 = (uint64_t)K_BLOCK_IDX * FM_NT; i0 < v.n_samples; i0 += stride) { // block-uniform
        PAR(tid) {
            const uint64_t i = i0 + tid;
            if (i < v.n_samples) {
                const uint64_t r = (uint64_t)STREAM_LOAD(&stage[i]), blk = r / G::ROWS;
                if (r <= v.n && blk < v.n_blocks) {
                    const uint32_t* p = v.occ + blk * G::BW;
                    const uint32_t k = (uint32_t)(r % G::ROWS);
                    uint32_t below = 0;
                    UNROLL
                    for (uint32_t w = 0; w < G::MWN; ++w) {
                        const uint32_t rows = k > 32 * w ? (k - 32 * w < 32 ? k - 32 * w : 32) : 0u;
                        const uint32_t mw = p[G::MW0 + w];
                        below += (uint32_t)__builtin_popcount(rows < 32 ? mw & ((1u << rows) - 1u) : mw);
                    }
                    const uint64_t si = (uint64_t)static_cast<const idx_t*>(v.mrank)[blk] + below;
                    if (si < v.n_samples) samples[si] = (idx_t)(i * v.s);
                }
            }
        }
    }
}


// ---- text-position samples and extract (capi_impl.h fm_add_text_samples_* / fm_extract_*; include/caps_sa_hip.h "FM-index: extract") --
// rowof[k] = the row of the suffix at text position k * t is the inverse of the SA samples at the multiples of t (s | t: every one of
// them is a sample), so it comes from the finished blob alone.  extract walks LF DOWN the text from the sample above a chunk of t
// positions: the stored code of the row of the suffix at e is T[e - 1].

// one lane per mark word: the samples of its marked rows (samples[mrank[block] + marks below], the locate kernel's rule); a sample
// v = k * t gives rowof[k] = the row.  Every sample index and every k is compared with its section's size before it is used.
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) fm_rowof_kernel(KCTX FmView v, uint32_t t, uint64_t m, idx_t* __restrict__ rowof)
{
    using G = FmGeom<idx_t>;
    const uint64_t words = v.n_blocks * G::MWN, stride = (uint64_t)K_GRID_DIM * FM_NT;
    const uint32_t sh = (uint32_t)__builtin_ctz(t | (FM_MAX_SAMPLE << 1));
    for (uint64_t w0 = (uint64_t)K_BLOCK_IDX * FM_NT; w0 < words; w0 += stride) {  // block-uniform
        PAR(tid) {
            const uint64_t w = w0 + tid;
            if (w < words) {
                const uint64_t blk = w / G::MWN;
                const uint32_t* p = v.occ + blk * G::BW + G::MW0;
                uint32_t mk = p[w % G::MWN];
                if (mk) {
                    uint64_t a = (uint64_t)static_cast<const idx_t*>(v.mrank)[blk];
                    for (uint32_t i = 0; i < (uint32_t)(w % G::MWN); ++i) a += (uint32_t)__builtin_popcount(p[i]);
                    while (mk) {
                        const uint32_t b = (uint32_t)__builtin_ctz(mk);
                        mk &= mk - 1;
                        const uint64_t r = w * FM_MROWS + b;
                        if (a < v.n_samples && r >= 1 && r <= v.n) {
                            const uint64_t val = (uint64_t)STREAM_LOAD(&static_cast<const idx_t*>(v.samples)[a]);
                            if ((val & (t - 1u)) == 0 && (val >> sh) < m) rowof[val >> sh] = (idx_t)r;
                        }
                        ++a;
                    }
                }
            }
        }
    }
}

// every rowof[k] is a row of the index, 1 .. n (a slot still 0: its sample is missing or stands twice) -- else flag 8
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) fm_rowof_check_kernel(KCTX const idx_t* __restrict__ rowof, uint64_t m, uint64_t n, uint32_t* __restrict__ flags)
{
    const uint64_t stride = (uint64_t)K_GRID_DIM * FM_NT;
    for (uint64_t k0 = (uint64_t)K_BLOCK_IDX * FM_NT; k0 < m; k0 += stride) {       // block-uniform
        PAR(tid) {
            const uint64_t k = k0 + tid;
            if (k < m) {
                const uint64_t r = (uint64_t)STREAM_LOAD(&rowof[k]);
                if (r == 0 || r > n) ATOMIC_OR_U32(flags, 8u);
            }
        }
    }
}

// extract's entry checks and plan: off[0 .. q] monotone (flag 1), start + len <= n without overflow (flag 2); cnt[j] = the chunks
// [k * t, (k + 1) * t) that query j touches (0 for an empty or refused one), scanned by fm_scan_kernel afterwards
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) fm_extract_plan_kernel(KCTX const uint64_t* __restrict__ start, const uint64_t* __restrict__ off, uint64_t q,
                                                       uint64_t n, uint32_t sh, uint64_t* __restrict__ cnt, uint32_t* __restrict__ flags)
{
    const uint64_t stride = (uint64_t)K_GRID_DIM * FM_NT;
    for (uint64_t j0 = (uint64_t)K_BLOCK_IDX * FM_NT; j0 < q; j0 += stride) {       // block-uniform
        PAR(tid) {
            const uint64_t j = j0 + tid;
            if (j < q) {
                const uint64_t a = off[j], b = off[j + 1], s = start[j], len = b >= a ? b - a : 0;
                uint32_t f = b < a ? 1u : 0u;
                if (s > n || len > n - s) f |= 2u;
                cnt[j] = !f && len ? ((s + len - 1) >> sh) - (s >> sh) + 1 : 0;
                if (f) ATOMIC_OR_U32(flags, f);
            }
        }
    }
}

// extract: one lane per (query, chunk) pair g in [0, lanes): its query j by bisection over the scanned chunk counts pre[0 .. q]
// (the locate kernel's over off), its chunk k = start / t + (g - pre[j]).  From E = min((k + 1) t, n), row rowof[k + 1] (row 0 for
// E = n: the suffix at n, L[0] = T[n - 1]), down to max(k t, start): at most t steps, each one block.  A byte goes out when its
// position lies below start + len.  WORDS: the letters are gathered in a register and an aligned 32-bit word of text is stored as
// one word only when all 4 of its bytes are this lane's; the bytes at both ends of the lane's range are byte stores (the
// neighbouring bytes belong to other lanes: never read, never rewritten).  flag 4: a rowof index outside its section, or the '$'
// row or row 0 met in mid-walk.
template <typename idx_t, bool WORDS>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) fm_extract_kernel(KCTX FmView v, const uint64_t* __restrict__ start, const uint64_t* __restrict__ off,
                                                  const uint64_t* __restrict__ pre, uint64_t q, uint64_t lanes, uint8_t* __restrict__ text,
                                                  uint32_t* __restrict__ flags)
{
    using G = FmGeom<idx_t>;
    const uint64_t stride = (uint64_t)K_GRID_DIM * FM_NT;
    const uint32_t sh = (uint32_t)__builtin_ctz(v.t | (FM_MAX_SAMPLE << 1));
    for (uint64_t g0 = (uint64_t)K_BLOCK_IDX * FM_NT; g0 < lanes; g0 += stride) {   // block-uniform
        PAR(tid) {
            const uint64_t g = g0 + tid;
            if (g < lanes) {
                uint64_t a = 0, b = q;                                              // the last j with pre[j] <= g
                while (b - a > 1) { const uint64_t mid = a + (b - a) / 2; if (pre[mid] <= g) a = mid; else b = mid; }
                const uint64_t s = start[a], o = off[a], o1 = off[a + 1], k = (s >> sh) + (g - pre[a]);
                if (pre[a] <= g && o1 >= o && s <= v.n && o1 - o <= v.n - s && k <= (v.n >> sh)) {
                    const uint64_t hi = s + (o1 - o), lo = std::max<uint64_t>(k << sh, s), E = std::min<uint64_t>((k + 1) << sh, v.n);
                    bool ok = true;
                    uint64_t r = 0;
                    if (E < v.n) {
                        if (k + 1 < v.n_text_samples) r = std::min<uint64_t>((uint64_t)static_cast<const idx_t*>(v.rowof)[k + 1], v.n);
                        else ok = false;
                    }
                    uint32_t acc = 0, have = 0;                                     // WORDS: the bytes gathered at wp .. wp + have - 1
                    uint8_t* wp = nullptr;
                    for (uint64_t e = E; ok && e > lo; --e) {
                        if (r == v.primary + 1 || (r == 0 && e != v.n)) { ok = false; break; }
                        const uint32_t* p = fm_block_of<idx_t>(v, r);
                        const uint32_t kk = (uint32_t)(r % G::ROWS);
                        const uint32_t c = (p[G::CW0 + kk / FM_WROWS] >> (2u * (kk % FM_WROWS))) & 3u;
                        if (e - 1 < hi) {
                            uint8_t* dst = text + o + (e - 1 - s);
                            const uint32_t letter = (v.syms >> (8u * c)) & 0xFFu;
                            if (WORDS) {
                                const uint32_t at = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u);
                                acc |= letter << (8u * at);
                                ++have;
                                wp = dst;
                                if (at == 0) {
                                    if (have == 4) *reinterpret_cast<uint32_t*>(dst) = acc;
                                    else for (uint32_t i = 0; i < have; ++i) dst[i] = (uint8_t)(acc >> (8u * i));
                                    acc = 0;
                                    have = 0;
                                }
                            } else {
                                *dst = (uint8_t)letter;
                            }
                        }
                        const uint64_t x = fm_c_of(v, c) + fm_block_occ<idx_t>(p, c, kk, r > v.primary + 1);
                        r = x <= v.n ? x : v.n;
                    }
                    if (WORDS && have) {
                        const uint32_t at = (uint32_t)(reinterpret_cast<uintptr_t>(wp) & 3u);
                        for (uint32_t i = 0; i < have; ++i) wp[i] = (uint8_t)(acc >> (8u * (at + i)));
                    }
                    if (!ok) ATOMIC_OR_U32(flags, 4u);
                }
            }
        }
    }
}

// ---- k-mers from SA and LCP (capi_impl.h kmer_*; include/caps_sa_hip.h "k-mers from SA and LCP") ---------------------------------
// Rank i is a head iff i == 0 or LCP[i] < k; a run is a head and the ranks up to the next head; a run whose head's suffix has k bytes
// (SA[h] <= n - k) is a distinct k-mer and its length the k-mer's count.  Tiles of FM_TILE ranks, FM_NT threads, grid-stride:
//   kmer_head_kernel    per tile the rank of its first head (n: none)
//   kmer_next_kernel    one workgroup: the suffix minimum over the tiles, next[t] = the first head at or after tile t, next[n_tiles] = n
//   kmer_run_kernel     per tile: coalesced 16-byte loads of LCP (and of SA where a chunk has a head) leave one byte per chunk in LDS
//                       -- its head bits and, 4 bits up, "this head's suffix has k bytes"; then a lane owns KMER_LANE consecutive
//                       ranks as a 64-bit mask, the first head behind the lane comes from a backward scan over the lanes' first
//                       heads in LDS and behind the tile from next[tile + 1]: no lane walks forward, whatever the run's length
//   kmer_census_kernel  one pass, every k at once: two difference histograms
// Nothing is indexed by a value read from SA or LCP except histogram bins, and those are compared with their bound first.
constexpr uint64_t KMER_TILE = FM_TILE;
constexpr uint32_t KMER_LANE = (uint32_t)(KMER_TILE / FM_NT);     // 64 ranks per lane: one mask word
constexpr uint32_t KMER_MAX_BINS = 1024;                          // spectrum bins, census max_k
constexpr uint32_t KMER_KEYS = KMER_MAX_BINS + 1;                 // columns of a histogram: bins 0 .. 1024
constexpr uint32_t KMER_CEN_COPIES = 4;                           // copies of the census histograms in LDS, one per lane mod 4
constexpr uint32_t KMER_GROUP = 16;                               // lanes of a group of the two-step scans over the lanes
enum { KMER_COUNT = 0, KMER_WRITE = 1, KMER_SPECTRUM = 2 };
static_assert(KMER_LANE == 64 && FM_NT == KMER_GROUP * KMER_GROUP, "a lane's ranks are one 64-bit mask; 16 groups of 16 lanes");
template <typename idx_t> struct KmerGeom {
    static constexpr uint32_t PER = 16u / sizeof(idx_t);                  // ranks of a 16-byte chunk (4 / 2)
    static constexpr uint32_t CHUNKS = (uint32_t)(KMER_TILE / PER);       // chunks of a tile
    static constexpr uint32_t ROUNDS = CHUNKS / FM_NT;                    // chunks per thread and tile (16 / 32)
    static constexpr uint32_t LANE_CHUNKS = KMER_LANE / PER;              // chunks of a lane's ranks
};
template <typename idx_t> struct alignas(sizeof(idx_t)) KmerChunk { idx_t v[16u / sizeof(idx_t)]; };

// ranks i0 .. i0 + PER - 1 (i0 < n): the entries of A that exist (the others 0)
template <typename idx_t>
HD KmerChunk<idx_t> kmer_load(const idx_t* __restrict__ A, uint64_t n, uint64_t i0)
{
    constexpr uint32_t PER = KmerGeom<idx_t>::PER;
    KmerChunk<idx_t> c;
    if (i0 + PER <= n) {
        c = *reinterpret_cast<const KmerChunk<idx_t>*>(A + i0);
    } else {
        for (uint32_t j = 0; j < PER; ++j) c.v[j] = i0 + j < n ? A[i0 + j] : (idx_t)0;
    }
    return c;
}
// the head bits of the chunk at i0 (i0 < n)
template <typename idx_t>
HD uint32_t kmer_head_bits(const idx_t* __restrict__ LCP, uint64_t n, uint64_t k, uint64_t i0)
{
    constexpr uint32_t PER = KmerGeom<idx_t>::PER;
    const KmerChunk<idx_t> c = kmer_load<idx_t>(LCP, n, i0);
    uint32_t hb = 0;
    UNROLL
    for (uint32_t j = 0; j < PER; ++j) hb |= (i0 + j < n && (uint64_t)c.v[j] < k ? 1u : 0u) << j;
    return i0 == 0 ? hb | 1u : hb;
}

template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) kmer_head_kernel(KCTX const idx_t* __restrict__ LCP, uint64_t n, uint64_t k, uint64_t n_tiles,
                                                 uint64_t* __restrict__ head)
{
    using G = KmerGeom<idx_t>;
    SHARED_ARRAY(uint32_t, first, 1);
    for (uint64_t tile = K_BLOCK_IDX; tile < n_tiles; tile += K_GRID_DIM) {         // block-uniform
        const uint64_t t0 = tile * KMER_TILE;
        PAR(tid) { if (tid == 0) first[0] = (uint32_t)KMER_TILE; }
        SYNC();
        PAR(tid) {
            // four chunks in flight, then a look: a lane stops at its first head (where nearly every rank is one, a genome at
            // k = 31, this pass reads a quarter of LCP; where none is, all of it)
            uint32_t best = (uint32_t)KMER_TILE;
            for (uint32_t j0 = 0; j0 < G::ROUNDS && best == (uint32_t)KMER_TILE; j0 += 4) {
                uint32_t hb[4];
                UNROLL
                for (uint32_t j = 0; j < 4; ++j) {
                    const uint64_t i0 = t0 + (uint64_t)((j0 + j) * FM_NT + tid) * G::PER;
                    hb[j] = i0 < n ? kmer_head_bits<idx_t>(LCP, n, k, i0) : 0u;
                }
                UNROLL
                for (uint32_t j = 0; j < 4; ++j)
                    if (hb[j] && best == (uint32_t)KMER_TILE) best = ((j0 + j) * FM_NT + tid) * G::PER + (uint32_t)__builtin_ctz(hb[j]);
            }
            if (best < (uint32_t)KMER_TILE) ATOMIC_MIN_U32(&first[0], best);
        }
        SYNC();
        PAR(tid) { if (tid == 0) head[tile] = first[0] < (uint32_t)KMER_TILE ? t0 + first[0] : n; }
        SYNC();
    }
}

// one workgroup, fm_scan_kernel's shape with min from the right: head[t] = the first head at or after tile t; head[n_tiles] = n
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) kmer_next_kernel(KCTX uint64_t* __restrict__ head, uint64_t n_tiles, uint64_t n)
{
    SHARED_ARRAY(uint64_t, part, FM_NT);
    const uint64_t per = (n_tiles + FM_NT - 1) / FM_NT;
    PAR(tid) {
        const uint64_t a = std::min<uint64_t>(n_tiles, tid * per), b = std::min<uint64_t>(n_tiles, a + per);
        uint64_t m = n;
        for (uint64_t t = a; t < b; ++t) m = std::min<uint64_t>(m, head[t]);
        part[tid] = m;
    }
    SYNC();
    PAR(tid) {
        if (tid == 0) {
            uint64_t m = n;
            for (uint32_t t = FM_NT; t-- > 0;) { const uint64_t v = part[t]; part[t] = m; m = std::min<uint64_t>(m, v); }
            head[n_tiles] = n;
        }
    }
    SYNC();
    PAR(tid) {
        const uint64_t a = std::min<uint64_t>(n_tiles, tid * per), b = std::min<uint64_t>(n_tiles, a + per);
        uint64_t m = part[tid];
        for (uint64_t t = b; t-- > a;) { m = std::min<uint64_t>(m, head[t]); head[t] = m; }
    }
}

// the runs whose heads are the bits of m (rank r0 + bit): f(head rank, length); behind the last one of the lane the run ends at lane_next
template <typename F>
DEV_INLINE void kmer_each_run(uint64_t m, uint64_t v, uint64_t r0, uint64_t lane_next, F&& f)
{
    while (m) {
        const uint32_t p = (uint32_t)__builtin_ctzll(m);
        m &= m - 1;
        const uint64_t h = r0 + p, e = m ? r0 + (uint32_t)__builtin_ctzll(m) : lane_next;
        if ((v >> p) & 1u) f(h, e - h);
    }
}

// MODE KMER_COUNT: cnt[tile] = the k-mers of the tile's heads with min_count <= count (<= max_count unless that is 0).
// MODE KMER_WRITE: cnt[] scanned (fm_scan_kernel); the same k-mers as records (first | count | pos) at cnt[tile] + their number in the
//                  tile, three 8-byte stores each; a slot at or beyond cap is not written.
// MODE KMER_SPECTRUM: every k-mer adds 1 to bin min(count, bins) of the workgroup's histogram; hist[bin * K_GRID_DIM + workgroup].
//                  Bin 1 (nearly every k-mer of a genome at k = 31) is counted in a register and added once per thread: no LDS
//                  atomic on the common path, and one copy of the histogram (4 KB) instead of eight.
template <typename idx_t, int MODE>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) kmer_run_kernel(KCTX const idx_t* __restrict__ SA, const idx_t* __restrict__ LCP, uint64_t n, uint64_t k,
                                                uint64_t n_tiles, const uint64_t* __restrict__ next, uint64_t min_count, uint64_t max_count,
                                                uint64_t* __restrict__ cnt, uint64_t* __restrict__ rec, uint64_t cap, uint32_t bins,
                                                uint64_t* __restrict__ hist)
{
    using G = KmerGeom<idx_t>;
    SHARED_ARRAY(uint8_t, bits, G::CHUNKS);                // per chunk: head bits | valid bits << 4
    SHARED_ARRAY(uint32_t, lane, FM_NT);                   // per lane: its first head (tile-relative; KMER_TILE: none), then its records
    SHARED_ARRAY(uint32_t, scan, FM_NT);                   // the scan of lane[] inside its group of 16, exclusive
    SHARED_ARRAY(uint32_t, grp, 2 * KMER_GROUP);           // per group: its min / sum, and the exclusive scan over the groups
    SHARED_ARRAY(uint32_t, h, MODE == KMER_SPECTRUM ? KMER_KEYS : 1);
    TL_DECL(uint64_t, st, 3);                              // a lane's head mask, valid mask, the first head behind its ranks
    TL_DECL(uint32_t, ones, 1);
    const uint64_t last_valid = k <= n ? n - k : 0;        // (k > n: no suffix has k bytes; the host never launches then)
    auto passes = [&](uint64_t c) { return c >= min_count && (max_count == 0 || c <= max_count); };
    PAR(tid) {
        TL(ones, tid, 0) = 0;
        if (MODE == KMER_SPECTRUM) for (uint32_t b = tid; b < KMER_KEYS; b += FM_NT) h[b] = 0;
    }
    SYNC();
    for (uint64_t tile = K_BLOCK_IDX; tile < n_tiles; tile += K_GRID_DIM) {         // block-uniform
        const uint64_t t0 = tile * KMER_TILE;
        PAR(tid) {
            if (tid == 0 && MODE == KMER_COUNT) h[0] = 0;
            UNROLL
            for (uint32_t j0 = 0; j0 < G::ROUNDS; j0 += 4) {
                uint32_t hb[4];
                UNROLL
                for (uint32_t j = 0; j < 4; ++j) {
                    const uint64_t i0 = t0 + (uint64_t)((j0 + j) * FM_NT + tid) * G::PER;
                    hb[j] = i0 < n ? kmer_head_bits<idx_t>(LCP, n, k, i0) : 0u;
                }
                UNROLL
                for (uint32_t j = 0; j < 4; ++j) {
                    const uint32_t c = (j0 + j) * FM_NT + tid;
                    uint32_t vb = 0;
                    if (hb[j] && k <= n) {
                        const uint64_t i0 = t0 + (uint64_t)c * G::PER;
                        const KmerChunk<idx_t> s = kmer_load<idx_t>(SA, n, i0);
                        UNROLL
                        for (uint32_t e = 0; e < G::PER; ++e) vb |= ((uint64_t)s.v[e] <= last_valid ? 1u : 0u) << e;
                        vb &= hb[j];
                    }
                    bits[c] = (uint8_t)(hb[j] | (vb << 4));
                }
            }
        }
        SYNC();
        PAR(tid) {
            uint64_t m = 0, v = 0;
            UNROLL
            for (uint32_t b = 0; b < G::LANE_CHUNKS; ++b) {
                const uint32_t x = bits[tid * G::LANE_CHUNKS + b];
                m |= (uint64_t)(x & 15u) << (b * G::PER);
                v |= (uint64_t)(x >> 4) << (b * G::PER);
            }
            TL(st, tid, 0) = m;
            TL(st, tid, 1) = v;
            lane[tid] = m ? tid * KMER_LANE + (uint32_t)__builtin_ctzll(m) : (uint32_t)KMER_TILE;
        }
        SYNC();
        PAR(tid) {                                          // backward: the first head behind every lane, inside its group
            if (tid < KMER_GROUP) {
                uint32_t run = (uint32_t)KMER_TILE;
                for (uint32_t j = KMER_GROUP; j-- > 0;) {
                    const uint32_t at = tid * KMER_GROUP + j, x = lane[at];
                    scan[at] = run;
                    run = std::min(run, x);
                }
                grp[tid] = run;
            }
        }
        SYNC();
        PAR(tid) {
            if (tid == 0) {
                uint32_t run = (uint32_t)KMER_TILE;
                for (uint32_t g = KMER_GROUP; g-- > 0;) { const uint32_t x = grp[g]; grp[KMER_GROUP + g] = run; run = std::min(run, x); }
            }
        }
        SYNC();
        PAR(tid) {
            const uint32_t nx = std::min(scan[tid], grp[KMER_GROUP + tid / KMER_GROUP]);
            const uint64_t lane_next = nx < (uint32_t)KMER_TILE ? t0 + nx : next[tile + 1];
            TL(st, tid, 2) = lane_next;
            const uint64_t r0 = t0 + (uint64_t)tid * KMER_LANE;
            if (MODE == KMER_SPECTRUM) {
                uint32_t one = 0;
                kmer_each_run(TL(st, tid, 0), TL(st, tid, 1), r0, lane_next, [&](uint64_t, uint64_t c) {
                    if (c == 1 || bins == 1) ++one;
                    else FETCH_ADD_U32(&h[c < bins ? (uint32_t)c : bins], 1u);
                });
                TL(ones, tid, 0) += one;
            } else {
                uint32_t mine = 0;
                kmer_each_run(TL(st, tid, 0), TL(st, tid, 1), r0, lane_next, [&](uint64_t, uint64_t c) { mine += passes(c) ? 1u : 0u; });
                if (MODE == KMER_COUNT) { if (mine) FETCH_ADD_U32(&h[0], mine); }
                else lane[tid] = mine;
            }
        }
        SYNC();
        if (MODE == KMER_COUNT) {
            PAR(tid) { if (tid == 0) cnt[tile] = h[0]; }
            SYNC();
        }
        if (MODE == KMER_WRITE) {
            PAR(tid) {                                      // forward: the records of the lanes before every lane
                if (tid < KMER_GROUP) {
                    uint32_t run = 0;
                    for (uint32_t j = 0; j < KMER_GROUP; ++j) {
                        const uint32_t at = tid * KMER_GROUP + j, x = lane[at];
                        scan[at] = run;
                        run += x;
                    }
                    grp[tid] = run;
                }
            }
            SYNC();
            PAR(tid) {
                if (tid == 0) {
                    uint32_t run = 0;
                    for (uint32_t g = 0; g < KMER_GROUP; ++g) { const uint32_t x = grp[g]; grp[KMER_GROUP + g] = run; run += x; }
                }
            }
            SYNC();
            PAR(tid) {
                uint64_t at = cnt[tile] + scan[tid] + grp[KMER_GROUP + tid / KMER_GROUP];
                const uint64_t r0 = t0 + (uint64_t)tid * KMER_LANE;
                kmer_each_run(TL(st, tid, 0), TL(st, tid, 1), r0, TL(st, tid, 2), [&](uint64_t hd, uint64_t c) {
                    if (!passes(c)) return;
                    if (at < cap) {
                        rec[3 * at] = hd;
                        rec[3 * at + 1] = c;
                        rec[3 * at + 2] = (uint64_t)SA[hd];
                    }
                    ++at;
                });
            }
            SYNC();
        }
    }
    if (MODE == KMER_SPECTRUM) {
        PAR(tid) { if (TL(ones, tid, 0)) FETCH_ADD_U32(&h[1], TL(ones, tid, 0)); }
        SYNC();
        PAR(tid) { for (uint32_t b = tid; b <= bins; b += FM_NT) hist[(uint64_t)b * K_GRID_DIM + K_BLOCK_IDX] = h[b]; }
    }
}

// census: rank i, with a = LCP[i] (0 at rank 0), a' = max(a, LCP[i + 1]) (0 behind the last rank) and b = n - SA[i] (0 for an SA[i] that
// is no position), adds 1 to distinct[k] for a < k <= b and to unique[k] for a' < k <= b -- as differences: +1 at bin lo + 1, -1 at
// bin b + 1, summed from the left on the host.  A bin above max_k is never read by that sum, so it is not counted at all (on a genome
// that is nearly every b + 1).  Two histograms of bins 0 .. max_k, KMER_CEN_COPIES copies each (copy = lane mod 4, bin-major, so the
// copies of a bin lie in four banks); hist[(which * KMER_KEYS + bin) * K_GRID_DIM + workgroup] = the copies' sum, two's complement.
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) kmer_census_kernel(KCTX const idx_t* __restrict__ SA, const idx_t* __restrict__ LCP, uint64_t n, uint32_t max_k,
                                                   uint64_t n_tiles, uint64_t* __restrict__ hist)
{
    using G = KmerGeom<idx_t>;
    constexpr uint32_t ONE = KMER_CEN_COPIES * KMER_KEYS;
    SHARED_ARRAY(uint32_t, d, 2 * ONE);
    PAR(tid) { for (uint32_t b = tid; b < 2 * ONE; b += FM_NT) d[b] = 0; }
    SYNC();
    for (uint64_t tile = K_BLOCK_IDX; tile < n_tiles; tile += K_GRID_DIM) {         // block-uniform
        const uint64_t t0 = tile * KMER_TILE;
        PAR(tid) {
            uint32_t* D = d + (tid % KMER_CEN_COPIES);
            auto add = [&](uint32_t* H, uint64_t a, uint64_t b) {
                if (a < b && a < max_k) {
                    FETCH_ADD_U32(&H[((uint32_t)a + 1u) * KMER_CEN_COPIES], 1u);
                    if (b < max_k) FETCH_ADD_U32(&H[((uint32_t)b + 1u) * KMER_CEN_COPIES], 0xFFFFFFFFu);
                }
            };
            for (uint32_t j = 0; j < G::ROUNDS; ++j) {
                const uint64_t i0 = t0 + (uint64_t)(j * FM_NT + tid) * G::PER;
                if (i0 >= n) break;
                const KmerChunk<idx_t> l = kmer_load<idx_t>(LCP, n, i0), s = kmer_load<idx_t>(SA, n, i0);
                const uint64_t behind = i0 + G::PER < n ? (uint64_t)LCP[i0 + G::PER] : 0;
                UNROLL
                for (uint32_t e = 0; e < G::PER; ++e) {
                    const uint64_t i = i0 + e;
                    if (i < n) {
                        const uint64_t a = i == 0 ? 0 : (uint64_t)l.v[e];
                        const uint64_t nx = e + 1 < G::PER ? (uint64_t)l.v[e + 1 < G::PER ? e + 1 : e] : behind;     // (0 behind rank n - 1)
                        const uint64_t b = (uint64_t)s.v[e] < n ? n - (uint64_t)s.v[e] : 0;
                        add(D, a, b);
                        add(D + ONE, std::max(a, nx), b);
                    }
                }
            }
        }
    }
    SYNC();
    PAR(tid) {
        for (uint32_t b = tid; b <= max_k; b += FM_NT) {
            for (uint32_t w = 0; w < 2; ++w) {
                int64_t s = 0;
                for (uint32_t c = 0; c < KMER_CEN_COPIES; ++c) s += (int32_t)d[w * ONE + b * KMER_CEN_COPIES + c];
                hist[((uint64_t)w * KMER_KEYS + b) * K_GRID_DIM + K_BLOCK_IDX] = (uint64_t)s;
            }
        }
    }
}

// ---- LPF and LZ77 from SA and LCP (capi_impl.h lpf_* / lz_*; include/caps_sa_hip.h "LPF and LZ77 from SA and LCP") -----------------------
// For rank r with i = SA[r]: p = the nearest rank below r whose SA value is below i, q = the nearest above; LPF[i] = the larger of
// min LCP(p, r] and min LCP(r, q].  A tree of fan-out LPF_F over the ranks holds (min SA, min LCP) of every node: level 1 = blocks of
// LPF_F ranks, level 2 = tiles of LPF_F blocks, and so on up to one node.  A search walks outwards over the siblings of its node, folds
// the min LCP of every node whose min SA >= i and climbs at the end of the group; the first node whose min SA < i holds the answer and
// the search descends through it, one group per level.  That is at most LPF_F steps per level and direction for ANY permutation; inside
// a tile the two lowest levels are in LDS.  A search ends early once its running minimum is 0 (left) or no larger than the left result
// (right: it cannot win any more).
//   lpf_block_kernel   level 1 from SA and LCP, coalesced 16-byte loads
//   lpf_up_kernel      level l from level l - 1 (one thread per parent; the levels above 1 are a 64th of the one below each)
//   lpf_tile_kernel    per tile: SA and LCP into LDS, the tile's block summaries beside them, one search pair per rank, two scattered
//                      stores; a search that leaves the tile goes on in lpf_far over the levels in global memory
// A value SA[r] >= n is never used as an index: the rank is skipped and *bad is raised.
//   lz_exit_kernel     per tile of LZ_TILE positions: ex[s] = the first position at or beyond the tile's end that the chain
//                      s -> s + len(s) reaches, by pointer doubling in LDS (the fixed point "the last chain position inside the tile")
//   lz_group_kernel    the exits composed over groups of LZ_GROUP tiles, for the first LZ_SPEC positions of every group, one lane each
//   lz_hop_kernel      one workgroup: the chain over the GROUPS, gentry[g] = where the parse enters group g (all-ones: it jumps over g);
//                      the composed exits of LZ_BATCH groups are fetched side by side before the lane walks them
//   lz_entry_kernel    one lane per group: from gentry[g] over the group's tiles, entry[t] = where the parse enters tile t
//   lz_walk_kernel     per tile with an entry: block exits right to left in LDS (one lane per block), one lane hops the blocks, then
//                      one lane per block walks at most LZ_BLOCK phrases: count / fm_scan_kernel / write, as kmer_run_kernel does
#if CAPS_TILE_E >= 4096
constexpr uint32_t LPF_SHIFT = 6;
#else
constexpr uint32_t LPF_SHIFT = 4;                                  // the small-tile emulation builds: blocks of 16, tiles of 256 ranks
#endif
constexpr uint32_t LPF_F = 1u << LPF_SHIFT;                        // fan-out of every level: ranks of a block, blocks of a tile
constexpr uint32_t LPF_TILE = LPF_F * LPF_F;                       // 4096 ranks: SA + LCP of a tile are 32 KiB (u32) / 64 KiB (u64) of LDS
constexpr uint32_t LPF_MAX_LEVELS = 16;                            // levels 1 .. 15 at most (n <= 2^60, fan-out >= 16)
constexpr uint32_t LZ_BLOCK = LPF_F;
constexpr uint32_t LZ_TILE = FM_NT * LZ_BLOCK;                     // 16,384 positions: one lane per block
constexpr uint32_t LZ_GROUP = LPF_F;                               // tiles of a group: the second level of the hop
constexpr uint64_t LZ_GPOS = (uint64_t)LZ_GROUP * LZ_TILE;         // 1,048,576 positions
constexpr uint32_t LZ_SPEC = 64;                                   // composed exits kept per group: its first positions
constexpr uint32_t LZ_BATCH = FM_NT;                               // groups fetched ahead at once
constexpr uint32_t LZ_ROUNDS = LPF_SHIFT + 8;                      // log2(LZ_TILE)
enum { LZ_COUNT = 0, LZ_WRITE = 1 };
static_assert(LZ_TILE == (1u << LZ_ROUNDS) && LZ_TILE <= 32768, "a tile-relative position and LZ_TILE itself fit 16 bits");

template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) lpf_block_kernel(KCTX const idx_t* __restrict__ SA, const idx_t* __restrict__ LCP, uint64_t n, uint64_t n_tiles,
                                                 uint64_t n_blocks, idx_t* __restrict__ sumSA, idx_t* __restrict__ sumLCP)
{
    constexpr uint32_t PER = KmerGeom<idx_t>::PER, CH = LPF_TILE / PER, CPB = LPF_F / PER;
    constexpr idx_t TOP = (idx_t)~(idx_t)0;
    SHARED_ARRAY(idx_t, cs, CH);
    SHARED_ARRAY(idx_t, cl, CH);
    for (uint64_t tile = K_BLOCK_IDX; tile < n_tiles; tile += K_GRID_DIM) {         // block-uniform
        const uint64_t t0 = tile * LPF_TILE;
        PAR(tid) {
            for (uint32_t c = tid; c < CH; c += FM_NT) {
                const uint64_t i0 = t0 + (uint64_t)c * PER;
                idx_t ms = TOP, ml = 0;
                if (i0 < n) {
                    const KmerChunk<idx_t> s = kmer_load<idx_t>(SA, n, i0), l = kmer_load<idx_t>(LCP, n, i0);
                    ml = TOP;
                    UNROLL
                    for (uint32_t j = 0; j < PER; ++j) {
                        const bool in = i0 + j < n;
                        ms = in && s.v[j] < ms ? s.v[j] : ms;
                        const idx_t lv = in && i0 + j != 0 ? l.v[j] : (idx_t)0;      // LCP[0] and what lies behind the array count as 0
                        ml = lv < ml ? lv : ml;
                    }
                }
                cs[c] = ms;
                cl[c] = ml;
            }
        }
        SYNC();
        PAR(tid) {
            for (uint32_t b = tid; b < LPF_F; b += FM_NT) {
                const uint64_t g = tile * LPF_F + b;
                if (g < n_blocks) {
                    idx_t ms = TOP, ml = TOP;
                    for (uint32_t c = 0; c < CPB; ++c) {
                        const idx_t a = cs[b * CPB + c], d = cl[b * CPB + c];
                        ms = a < ms ? a : ms;
                        ml = d < ml ? d : ml;
                    }
                    sumSA[g] = ms;
                    sumLCP[g] = ml;
                }
            }
        }
        SYNC();
    }
}

// parents [0, n_par) at par_off from the children [0, n_child) at child_off of the same two arrays
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) lpf_up_kernel(KCTX idx_t* __restrict__ sumSA, idx_t* __restrict__ sumLCP, uint64_t child_off, uint64_t n_child,
                                              uint64_t par_off, uint64_t n_par)
{
    constexpr idx_t TOP = (idx_t)~(idx_t)0;
    PAR(tid) {
        for (uint64_t p = (uint64_t)K_BLOCK_IDX * FM_NT + tid; p < n_par; p += (uint64_t)K_GRID_DIM * FM_NT) {
            const uint64_t c0 = p * LPF_F, c1 = std::min<uint64_t>(n_child, c0 + LPF_F);
            idx_t ms = TOP, ml = TOP;
            for (uint64_t c = c0; c < c1; ++c) {
                const idx_t a = sumSA[child_off + c], d = sumLCP[child_off + c];
                ms = a < ms ? a : ms;
                ml = d < ml ? d : ml;
            }
            sumSA[par_off + p] = ms;
            sumLCP[par_off + p] = ml;
        }
    }
}

// The search of value i beyond its tile: `pos` = its tile (a node of level 2), m = the minimum so far.  Ascends over the siblings at
// levels 2 .. top, descends through the first node whose min SA < i.  tab[2 l] / tab[2 l + 1] = offset / nodes of level l.  Ends as
// soon as m <= stop (found stays false: the caller's result is then 0).  found: val = the SA value, m = the minimum.
template <typename idx_t, bool RIGHT>
DEV_INLINE void lpf_far(const idx_t* __restrict__ SA, const idx_t* __restrict__ LCP, uint64_t n, const idx_t* __restrict__ sumSA,
                        const idx_t* __restrict__ sumLCP, const uint64_t* __restrict__ tab, uint32_t top, uint64_t pos, idx_t i, idx_t stop,
                        idx_t& m, bool& found, idx_t& val)
{
    uint32_t lev = 2;
    uint64_t hit = 0;
    bool have = false;
    while (lev <= top && !have) {
        const uint64_t off = tab[2 * lev], cnt = tab[2 * lev + 1];
        const uint64_t lo = pos & ~(uint64_t)(LPF_F - 1), hi = std::min<uint64_t>(cnt, lo + LPF_F);
        for (uint64_t k = 1; k < LPF_F; ++k) {
            if (RIGHT ? pos + k >= hi : pos < lo + k) break;
            const uint64_t j = RIGHT ? pos + k : pos - k;
            if (sumSA[off + j] < i) { have = true; hit = j; break; }
            const idx_t d = sumLCP[off + j];
            m = d < m ? d : m;
            if (m <= stop) return;
        }
        if (!have) { pos >>= LPF_SHIFT; ++lev; }
    }
    if (!have) return;
    while (lev > 1) {                                                               // into the children at level lev - 1
        --lev;
        const uint64_t off = tab[2 * lev], cnt = tab[2 * lev + 1];
        const uint64_t c0 = hit * LPF_F, c1 = std::min<uint64_t>(cnt, c0 + LPF_F);
        have = false;
        for (uint64_t k = 0; c0 + k < c1; ++k) {
            const uint64_t j = RIGHT ? c0 + k : c1 - 1 - k;
            if (sumSA[off + j] < i) { have = true; hit = j; break; }
            const idx_t d = sumLCP[off + j];
            m = d < m ? d : m;
            if (m <= stop) return;
        }
        if (!have) return;                                                          // (a summary and its children disagree: no answer)
    }
    const uint64_t c0 = hit * LPF_F, c1 = std::min<uint64_t>(n, c0 + LPF_F);        // the ranks of the block
    for (uint64_t k = 0; c0 + k < c1; ++k) {
        const uint64_t j = RIGHT ? c0 + k : c1 - 1 - k;
        const idx_t s = SA[j], d = j ? LCP[j] : (idx_t)0;
        if (RIGHT) {
            m = d < m ? d : m;
            if (m <= stop) return;
            if (s < i) { found = true; val = s; return; }
        } else {
            if (s < i) { found = true; val = s; return; }
            m = d < m ? d : m;
            if (m <= stop) return;
        }
    }
}

template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) lpf_tile_kernel(KCTX const idx_t* __restrict__ SA, const idx_t* __restrict__ LCP, uint64_t n, uint64_t n_tiles,
                                                uint64_t n_blocks, const idx_t* __restrict__ sumSA, const idx_t* __restrict__ sumLCP,
                                                const uint64_t* __restrict__ tab, uint32_t top, idx_t* __restrict__ LPF, idx_t* __restrict__ Prev,
                                                uint32_t* __restrict__ bad)
{
    constexpr uint32_t PER = KmerGeom<idx_t>::PER, CH = LPF_TILE / PER;
    constexpr idx_t TOP = (idx_t)~(idx_t)0;
    SHARED_ARRAY(idx_t, sSA, LPF_TILE);
    SHARED_ARRAY(idx_t, sLCP, LPF_TILE);
    SHARED_ARRAY(idx_t, bSA, LPF_F);
    SHARED_ARRAY(idx_t, bLCP, LPF_F);
    for (uint64_t tile = K_BLOCK_IDX; tile < n_tiles; tile += K_GRID_DIM) {         // block-uniform
        const uint64_t t0 = tile * LPF_TILE;
        PAR(tid) {
            for (uint32_t c = tid; c < CH; c += FM_NT) {
                const uint64_t i0 = t0 + (uint64_t)c * PER;
                KmerChunk<idx_t> s{}, l{};
                if (i0 < n) {
                    s = kmer_load<idx_t>(SA, n, i0);
                    l = kmer_load<idx_t>(LCP, n, i0);
                }
                UNROLL
                for (uint32_t j = 0; j < PER; ++j) {
                    const bool in = i0 + j < n;
                    sSA[c * PER + j] = in ? s.v[j] : TOP;                            // behind the array: never below i, and a 0 that ends the search
                    sLCP[c * PER + j] = in && i0 + j != 0 ? l.v[j] : (idx_t)0;
                }
            }
            for (uint32_t b = tid; b < LPF_F; b += FM_NT) {
                const uint64_t g = tile * LPF_F + b;
                bSA[b] = g < n_blocks ? sumSA[g] : TOP;
                bLCP[b] = g < n_blocks ? sumLCP[g] : (idx_t)0;
            }
        }
        SYNC();
        PAR(tid) {
            for (uint32_t x = tid; x < LPF_TILE; x += FM_NT) {
                if (t0 + x >= n) break;
                const idx_t i = sSA[x];
                if ((uint64_t)i >= n) { ATOMIC_MAX_U32(bad, 1u); continue; }
                // left: p < r, min LCP(p, r]
                idx_t m = sLCP[x], pv = TOP;
                bool found = false;
                if (m != 0) {
                    bool out = true;                                                // no node below i seen yet, m still above 0
                    uint32_t j = x;
                    while (j & (LPF_F - 1)) {
                        --j;
                        if (sSA[j] < i) { found = true; pv = sSA[j]; out = false; break; }
                        const idx_t d = sLCP[j];
                        m = d < m ? d : m;
                        if (m == 0) { out = false; break; }
                    }
                    uint32_t b = x >> LPF_SHIFT;
                    while (out && b) {
                        --b;
                        if (bSA[b] < i) {
                            out = false;
                            for (j = (b + 1) * LPF_F; j-- > b * LPF_F;) {
                                if (sSA[j] < i) { found = true; pv = sSA[j]; break; }
                                const idx_t d = sLCP[j];
                                m = d < m ? d : m;
                                if (m == 0) break;
                            }
                        } else {
                            const idx_t d = bLCP[b];
                            m = d < m ? d : m;
                            if (m == 0) out = false;
                        }
                    }
                    if (out && tile) lpf_far<idx_t, false>(SA, LCP, n, sumSA, sumLCP, tab, top, tile, i, (idx_t)0, m, found, pv);
                }
                const idx_t left = found ? m : (idx_t)0;
                // right: q > r, min LCP(r, q]; it wins only if it is larger than left
                idx_t qv = TOP;
                m = TOP;
                found = false;
                if (left != TOP) {
                    bool out = true;
                    uint32_t j = x;
                    while ((j + 1) & (LPF_F - 1)) {
                        ++j;
                        const idx_t d = sLCP[j];
                        m = d < m ? d : m;
                        if (m <= left) { out = false; break; }
                        if (sSA[j] < i) { found = true; qv = sSA[j]; out = false; break; }
                    }
                    uint32_t b = x >> LPF_SHIFT;
                    while (out && b + 1 < LPF_F) {
                        ++b;
                        if (bSA[b] < i) {
                            out = false;
                            for (j = b * LPF_F; j < (b + 1) * LPF_F; ++j) {
                                const idx_t d = sLCP[j];
                                m = d < m ? d : m;
                                if (m <= left) break;
                                if (sSA[j] < i) { found = true; qv = sSA[j]; break; }
                            }
                        } else {
                            const idx_t d = bLCP[b];
                            m = d < m ? d : m;
                            if (m <= left) out = false;
                        }
                    }
                    if (out && tile + 1 < n_tiles) lpf_far<idx_t, true>(SA, LCP, n, sumSA, sumLCP, tab, top, tile, i, left, m, found, qv);
                }
                const idx_t right = found ? m : (idx_t)0;
                idx_t len = 0, src = TOP;
                if (right > left) { len = right; src = qv; }
                else if (left > 0) { len = left; src = pv; }
                if (LPF) LPF[i] = len;
                if (Prev) Prev[i] = src;
            }
        }
        SYNC();
    }
}

// the phrase at position s (s < n): max(1, LPF[s]) clamped to the text's end
HD uint64_t lz_len(uint64_t lpf, uint64_t n, uint64_t s) { return std::min<uint64_t>(lpf ? lpf : 1, n - s); }

template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) lz_exit_kernel(KCTX const idx_t* __restrict__ LPF, uint64_t n, uint64_t n_tiles, idx_t* __restrict__ ex)
{
    SHARED_ARRAY(uint16_t, bufa, LZ_TILE);
    SHARED_ARRAY(uint16_t, bufb, LZ_TILE);
    for (uint64_t tile = K_BLOCK_IDX; tile < n_tiles; tile += K_GRID_DIM) {         // block-uniform
        const uint64_t t0 = tile * LZ_TILE;
        PAR(tid) {
            for (uint32_t s = tid; s < LZ_TILE; s += FM_NT) {
                const uint64_t pos = t0 + s;
                uint32_t nx = s;                                                    // the fixed point: the chain leaves the tile from here
                if (pos < n) {
                    const uint64_t len = lz_len((uint64_t)LPF[pos], n, pos);
                    if (len < LZ_TILE - s && pos + len < n) nx = s + (uint32_t)len;
                }
                bufa[s] = (uint16_t)nx;
            }
        }
        SYNC();
        uint16_t* src = bufa;
        uint16_t* dst = bufb;
        for (uint32_t r = 0; r < LZ_ROUNDS; ++r) {
            PAR(tid) { for (uint32_t s = tid; s < LZ_TILE; s += FM_NT) dst[s] = src[src[s]]; }
            SYNC();
            uint16_t* t = src; src = dst; dst = t;
        }
        PAR(tid) {
            for (uint32_t s = tid; s < LZ_TILE; s += FM_NT) {
                const uint64_t pos = t0 + s;
                if (pos < n) {
                    const uint64_t last = t0 + src[s];                              // (>= pos, < n: the chain never passes n)
                    ex[pos] = (idx_t)(last + lz_len((uint64_t)LPF[last], n, last));
                }
            }
        }
        SYNC();
    }
}

// gx[g * LZ_SPEC + o] = where the chain from position g * LZ_GPOS + o leaves group g: the exits of at most LZ_GROUP tiles composed,
// for the first LZ_SPEC positions of every group, one lane each
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) lz_group_kernel(KCTX const idx_t* __restrict__ ex, uint64_t n, uint64_t n_groups, idx_t* __restrict__ gx)
{
    PAR(tid) {
        for (uint64_t k = (uint64_t)K_BLOCK_IDX * FM_NT + tid; k < n_groups * LZ_SPEC; k += (uint64_t)K_GRID_DIM * FM_NT) {
            const uint64_t g = k / LZ_SPEC, end = std::min<uint64_t>(n, (g + 1) * LZ_GPOS);
            uint64_t e = g * LZ_GPOS + k % LZ_SPEC;
            for (uint32_t hop = 0; hop < LZ_GROUP && e < end; ++hop) {              // (an exit lies beyond its tile: a hop per tile at most)
                const uint64_t nx = (uint64_t)ex[e];
                e = nx > e ? nx : n;
            }
            gx[k] = (idx_t)std::min<uint64_t>(e, n);
        }
    }
}

// one workgroup: the chain over the GROUPS, gentry[g] = the position at which the parse enters group g (all-ones: it jumps over g).
// The composed exits of LZ_BATCH groups go into LDS before the lane walks them; an entry at LZ_SPEC or more positions into its group
// hops the group's tiles instead (at most LZ_GROUP dependent loads).
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) lz_hop_kernel(KCTX const idx_t* __restrict__ ex, const idx_t* __restrict__ gx, uint64_t n, uint64_t n_groups,
                                              uint64_t* __restrict__ gentry)
{
    SHARED_ARRAY(idx_t, spec, LZ_BATCH * LZ_SPEC);
    SHARED_ARRAY(uint64_t, st, 1);
    PAR(tid) {
        for (uint64_t g = tid; g < n_groups; g += FM_NT) gentry[g] = ~(uint64_t)0;
        if (tid == 0) st[0] = 0;
    }
    SYNC();
    for (uint64_t base = 0; base < n_groups; base += LZ_BATCH) {                    // block-uniform
        PAR(tid) {
            if (st[0] / LZ_GPOS < base + LZ_BATCH) {                                // (else the chain jumps over the whole batch)
                for (uint32_t k = tid; k < LZ_BATCH * LZ_SPEC; k += FM_NT) {
                    const uint64_t at = base * LZ_SPEC + k;
                    spec[k] = at < n_groups * LZ_SPEC ? gx[at] : (idx_t)0;
                }
            }
        }
        SYNC();
        PAR(tid) {
            if (tid == 0) {
                uint64_t e = st[0];
                while (e < n) {
                    const uint64_t g = e / LZ_GPOS;
                    if (g >= base + LZ_BATCH) break;
                    gentry[g] = e;
                    const uint64_t off = e - g * LZ_GPOS;
                    uint64_t nx = e;
                    if (off < LZ_SPEC) {
                        nx = (uint64_t)spec[(g - base) * LZ_SPEC + off];
                    } else {
                        const uint64_t end = std::min<uint64_t>(n, (g + 1) * LZ_GPOS);
                        for (uint32_t hop = 0; hop < LZ_GROUP && nx < end; ++hop) {
                            const uint64_t t = (uint64_t)ex[nx];
                            nx = t > nx ? t : n;
                        }
                    }
                    e = nx > e ? nx : n;                                            // (always forward)
                }
                st[0] = e;
            }
        }
        SYNC();
    }
}

// one lane per group: entry[t] for the group's tiles (all-ones: the parse jumps over t), at most LZ_GROUP dependent loads
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) lz_entry_kernel(KCTX const idx_t* __restrict__ ex, uint64_t n, uint64_t n_tiles, uint64_t n_groups,
                                                const uint64_t* __restrict__ gentry, uint64_t* __restrict__ entry)
{
    PAR(tid) {
        for (uint64_t g = (uint64_t)K_BLOCK_IDX * FM_NT + tid; g < n_groups; g += (uint64_t)K_GRID_DIM * FM_NT) {
            const uint64_t t1 = std::min<uint64_t>(n_tiles, (g + 1) * LZ_GROUP), end = std::min<uint64_t>(n, (g + 1) * LZ_GPOS);
            for (uint64_t t = g * LZ_GROUP; t < t1; ++t) entry[t] = ~(uint64_t)0;
            uint64_t e = gentry[g];
            if (e < g * LZ_GPOS) e = end;                                           // (all-ones is beyond `end` anyway)
            for (uint32_t hop = 0; hop < LZ_GROUP && e < end; ++hop) {
                entry[e / LZ_TILE] = e;
                const uint64_t nx = (uint64_t)ex[e];
                e = nx > e ? nx : n;
            }
        }
    }
}

// MODE LZ_COUNT: cnt[tile] = the phrases that start in the tile.  MODE LZ_WRITE: cnt[] scanned; the records (pos | len | src) at
// cnt[tile] + their number in the tile; a slot at or beyond cap is not written.
template <typename idx_t, int MODE>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) lz_walk_kernel(KCTX const idx_t* __restrict__ LPF, const idx_t* __restrict__ Prev, uint64_t n, uint64_t n_tiles,
                                               const uint64_t* __restrict__ entry, uint64_t* __restrict__ cnt, uint64_t* __restrict__ rec,
                                               uint64_t cap)
{
    SHARED_ARRAY(uint16_t, nxt, LZ_TILE);                  // the next phrase's start, tile-relative; LZ_TILE: beyond the tile or the text
    SHARED_ARRAY(uint16_t, bx, LZ_TILE);                   // the first chain position beyond the block
    SHARED_ARRAY(uint16_t, bent, FM_NT);                   // per block: where the parse enters it (LZ_TILE: nowhere)
    SHARED_ARRAY(uint32_t, lane, FM_NT);
    SHARED_ARRAY(uint32_t, scan, FM_NT);
    SHARED_ARRAY(uint32_t, grp, 2 * KMER_GROUP);
    SHARED_ARRAY(uint32_t, h, 1);
    for (uint64_t tile = K_BLOCK_IDX; tile < n_tiles; tile += K_GRID_DIM) {         // block-uniform
        const uint64_t t0 = tile * LZ_TILE, e = entry[tile];
        if (e < t0 || e - t0 >= LZ_TILE || e >= n) {                                // the parse jumps over this tile
            if (MODE == LZ_COUNT) { PAR(tid) { if (tid == 0) cnt[tile] = 0; } }
            continue;
        }
        PAR(tid) {
            for (uint32_t s = tid; s < LZ_TILE; s += FM_NT) {
                const uint64_t pos = t0 + s;
                uint32_t nx = LZ_TILE;
                if (pos < n) {
                    const uint64_t len = lz_len((uint64_t)LPF[pos], n, pos);
                    if (len < LZ_TILE - s && pos + len < n) nx = s + (uint32_t)len;
                }
                nxt[s] = (uint16_t)nx;
            }
            bent[tid] = (uint16_t)LZ_TILE;
            if (tid == 0) h[0] = 0;
        }
        SYNC();
        PAR(tid) {                                          // one lane per block, right to left
            const uint32_t b0 = tid * LZ_BLOCK, b1 = b0 + LZ_BLOCK;
            for (uint32_t s = b1; s-- > b0;) {
                const uint32_t v = nxt[s];
                bx[s] = v >= b1 ? (uint16_t)v : bx[v];
            }
        }
        SYNC();
        PAR(tid) {
            if (tid == 0) {
                uint32_t cur = (uint32_t)(e - t0);
                while (cur < LZ_TILE) {
                    bent[cur / LZ_BLOCK] = (uint16_t)cur;
                    const uint32_t v = bx[cur];
                    cur = v > cur ? v : LZ_TILE;
                }
            }
        }
        SYNC();
        PAR(tid) {
            const uint32_t b1 = (tid + 1) * LZ_BLOCK;
            uint32_t mine = 0;
            for (uint32_t cur = bent[tid]; cur < b1; cur = nxt[cur]) ++mine;
            if (MODE == LZ_COUNT) { if (mine) FETCH_ADD_U32(&h[0], mine); }
            else lane[tid] = mine;
        }
        SYNC();
        if (MODE == LZ_COUNT) {
            PAR(tid) { if (tid == 0) cnt[tile] = h[0]; }
            SYNC();
        } else {
            PAR(tid) {                                      // forward: the records of the lanes before every lane
                if (tid < KMER_GROUP) {
                    uint32_t run = 0;
                    for (uint32_t j = 0; j < KMER_GROUP; ++j) {
                        const uint32_t at = tid * KMER_GROUP + j, x = lane[at];
                        scan[at] = run;
                        run += x;
                    }
                    grp[tid] = run;
                }
            }
            SYNC();
            PAR(tid) {
                if (tid == 0) {
                    uint32_t run = 0;
                    for (uint32_t g = 0; g < KMER_GROUP; ++g) { const uint32_t x = grp[g]; grp[KMER_GROUP + g] = run; run += x; }
                }
            }
            SYNC();
            PAR(tid) {
                const uint32_t b1 = (tid + 1) * LZ_BLOCK;
                uint64_t at = cnt[tile] + scan[tid] + grp[KMER_GROUP + tid / KMER_GROUP];
                for (uint32_t cur = bent[tid]; cur < b1; cur = nxt[cur]) {
                    const uint64_t pos = t0 + cur, lp = (uint64_t)LPF[pos];
                    if (at < cap) {
                        rec[3 * at] = pos;
                        rec[3 * at + 1] = lz_len(lp, n, pos);
                        rec[3 * at + 2] = lp ? (uint64_t)Prev[pos] : ~(uint64_t)0;
                    }
                    ++at;
                }
            }
            SYNC();
        }
    }
}

// ---- ISA and the LCE index (capi_impl.h isa_* / lce_*; include/caps_sa_hip.h "ISA and longest common extensions") ----------------------
// ISA[SA[r]] = r, and an index that answers range_min(lo, hi) = min LCP[lo .. hi] over ranks and, from it, the longest common extension
// of two text positions with up to k mismatches (kangaroo jumps).  The blob holds ISA, a copy of LCP with entry 0 stored as 0, and two
// tiers of sparse tables: M_j[b] = the minimum of the blocks b .. b + 2^j - 1 (blocks of LCE_BLOCK ranks, j = 0 .. 6) and T_j[s] = the
// minimum of the superblocks s .. s + 2^j - 1 (LCE_SUPER ranks, j = 0 .. floor(log2 ns)), both clipped at the end of the array.
//   isa_scatter_kernel    SA streamed with 16-byte loads, one scattered store per rank into a destination preset to all ones; a value
//                         >= n is never used as an index and raises bit 0 of *bad
//   isa_check_kernel      streams the destination: a slot that is still all ones raises bit 1 (with n in-range stores, no empty slot
//                         means a permutation: a duplicate leaves a slot empty)
//   lce_block_kernel      one pass over LCP: the copy and M_0, the chunk minima through LDS (lpf_block_kernel's shape)
//   lce_table_kernel      one level from another: dst[x] = min(src[x * mul], src[x * mul + half]) -- M_j from M_{j-1} (mul 1, half
//                         2^(j-1)), T_0 from M_6 at superblock starts (mul 64, half 0), T_j from T_{j-1}
//   lce_range_min_kernel  one lane per query: the two partial blocks by 16-byte loads (single entries only at their unaligned ends), the
//   lce_query_kernel      whole blocks between them by two overlapping reads of M_j, or by M_j up to the next superblock edge, T_j over
//                         the whole superblocks, M_j from the last edge: at most 126 LCP reads and 6 table reads for ANY blob body; a
//                         round of lce adds 2 ISA reads, clamped to n - 1.  Nothing walks a data-dependent distance.
// LCE_BLOCK and LCE_SUPER are the blob's format: the same in every build, the small-tile emulation builds included.
constexpr uint32_t LCE_BLOCK = 64;
constexpr uint32_t LCE_SUPER = 4096;
constexpr uint32_t LCE_BPS = LCE_SUPER / LCE_BLOCK;               // blocks of a superblock
constexpr uint32_t LCE_MLEVELS = 7;                               // M_0 .. M_6: runs of up to 64 blocks
constexpr uint32_t LCE_MAX_TLEVELS = 64;
constexpr uint32_t LCE_MAX_MISMATCHES = 1024;
static_assert(LCE_BPS == (1u << (LCE_MLEVELS - 1)), "M_6 at a superblock start is the superblock");

// the kernels' view of a checked blob (capi_impl.h lce_check_header): section pointers, strides between the levels in bytes
struct LceView {
    uint64_t n = 0, nb = 0, ns = 0;
    uint32_t tlevels = 0;                                          // T_0 .. T_{tlevels - 1}
    const char* isa = nullptr;
    const char* lcp = nullptr;
    const char* m = nullptr;
    const char* t = nullptr;
    uint64_t m_stride = 0, t_stride = 0;
};

template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) isa_scatter_kernel(KCTX const idx_t* __restrict__ SA, uint64_t n, idx_t* __restrict__ ISA, uint32_t* __restrict__ bad)
{
    constexpr uint32_t PER = KmerGeom<idx_t>::PER;
    const uint64_t chunks = (n + PER - 1) / PER;
    PAR(tid) {
        for (uint64_t c = (uint64_t)K_BLOCK_IDX * FM_NT + tid; c < chunks; c += (uint64_t)K_GRID_DIM * FM_NT) {
            const uint64_t i0 = c * PER;
            const KmerChunk<idx_t> s = kmer_load<idx_t>(SA, n, i0);
            UNROLL
            for (uint32_t j = 0; j < PER; ++j) {
                if (i0 + j >= n) break;
                const uint64_t v = (uint64_t)s.v[j];
                if (v < n) ISA[v] = (idx_t)(i0 + j);
                else ATOMIC_OR_U32(bad, 1u);
            }
        }
    }
}

template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) isa_check_kernel(KCTX const idx_t* __restrict__ ISA, uint64_t n, uint32_t* __restrict__ bad)
{
    constexpr uint32_t PER = KmerGeom<idx_t>::PER;
    constexpr idx_t TOP = (idx_t)~(idx_t)0;
    const uint64_t chunks = (n + PER - 1) / PER;
    PAR(tid) {
        bool empty = false;
        for (uint64_t c = (uint64_t)K_BLOCK_IDX * FM_NT + tid; c < chunks; c += (uint64_t)K_GRID_DIM * FM_NT) {
            const uint64_t i0 = c * PER;
            const KmerChunk<idx_t> s = kmer_load<idx_t>(ISA, n, i0);
            UNROLL
            for (uint32_t j = 0; j < PER; ++j) empty = empty || (i0 + j < n && s.v[j] == TOP);
        }
        if (empty) ATOMIC_OR_U32(bad, 2u);
    }
}

template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) lce_block_kernel(KCTX const idx_t* __restrict__ LCP, uint64_t n, uint64_t n_tiles, uint64_t nb,
                                                 idx_t* __restrict__ copy, idx_t* __restrict__ M0)
{
    constexpr uint32_t PER = KmerGeom<idx_t>::PER, CH = LCE_SUPER / PER, CPB = LCE_BLOCK / PER;
    constexpr idx_t TOP = (idx_t)~(idx_t)0;
    SHARED_ARRAY(idx_t, cl, CH);
    for (uint64_t tile = K_BLOCK_IDX; tile < n_tiles; tile += K_GRID_DIM) {         // block-uniform
        const uint64_t t0 = tile * LCE_SUPER;
        PAR(tid) {
            for (uint32_t c = tid; c < CH; c += FM_NT) {
                const uint64_t i0 = t0 + (uint64_t)c * PER;
                idx_t ml = TOP;
                if (i0 < n) {
                    KmerChunk<idx_t> l = kmer_load<idx_t>(LCP, n, i0);
                    if (i0 == 0) l.v[0] = 0;                                         // LCP[0] counts as 0 and is stored as 0
                    UNROLL
                    for (uint32_t j = 0; j < PER; ++j) ml = i0 + j < n && l.v[j] < ml ? l.v[j] : ml;
                    if (i0 + PER <= n) {
                        *reinterpret_cast<KmerChunk<idx_t>*>(copy + i0) = l;
                    } else {
                        for (uint32_t j = 0; i0 + j < n; ++j) copy[i0 + j] = l.v[j];
                    }
                }
                cl[c] = ml;
            }
        }
        SYNC();
        PAR(tid) {
            for (uint32_t b = tid; b < LCE_BPS; b += FM_NT) {
                const uint64_t g = tile * LCE_BPS + b;
                if (g < nb) {
                    idx_t ml = TOP;
                    for (uint32_t c = 0; c < CPB; ++c) {
                        const idx_t d = cl[b * CPB + c];
                        ml = d < ml ? d : ml;
                    }
                    M0[g] = ml;
                }
            }
        }
        SYNC();
    }
}

// dst[x] = min(src[x * mul], src[x * mul + half]) for x < n_dst; the second only where half != 0 and it exists
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) lce_table_kernel(KCTX const idx_t* __restrict__ src, uint64_t n_src, idx_t* __restrict__ dst, uint64_t n_dst,
                                                 uint64_t mul, uint64_t half)
{
    PAR(tid) {
        for (uint64_t x = (uint64_t)K_BLOCK_IDX * FM_NT + tid; x < n_dst; x += (uint64_t)K_GRID_DIM * FM_NT) {
            const uint64_t a = x * mul;
            if (a >= n_src) continue;                                                // (never, for the shapes the host launches)
            idx_t m = src[a];
            if (half && a + half < n_src) {
                const idx_t d = src[a + half];
                m = d < m ? d : m;
            }
            dst[x] = m;
        }
    }
}

// min of m and LCP over two rank ranges [a0, e0) and [a1, e1), each inside one block and inside the array, either may be empty: single
// entries up to the first 16-byte edge and behind the last, 16-byte chunks between.  A query is a chain of dependent rounds (load,
// wait, fold), and a wave makes as many as its slowest lane.  So the two ranges share their rounds; the single entries of all four ends
// are loaded up front and folded last; and the chunks go U at a time per range, in order (taking every R-th chunk per round instead, so
// that the first round touches every line, was measured and is slower: a range of 8 chunks then needs 4 rounds, not 2).
template <typename idx_t>
DEV_INLINE idx_t lce_scan2(const idx_t* __restrict__ lcp, uint64_t a0, uint64_t e0, uint64_t a1, uint64_t e1, idx_t m)
{
    constexpr uint32_t PER = KmerGeom<idx_t>::PER, U = 4;
    constexpr idx_t TOP = (idx_t)~(idx_t)0;
    const uint64_t lo[2] = {a0, a1}, hi[2] = {e0 > a0 ? e0 : a0, e1 > a1 ? e1 : a1};
    uint64_t c0[2], c1[2];                                                          // the whole chunks of a range are [c0, c1)
    idx_t v[2][2][PER];
    UNROLL
    for (uint32_t r = 0; r < 2; ++r) {
        const uint64_t edge = (lo[r] + PER - 1) & ~(uint64_t)(PER - 1);
        c0[r] = edge < hi[r] ? edge : hi[r];
        c1[r] = c0[r] + ((hi[r] - c0[r]) & ~(uint64_t)(PER - 1));
        UNROLL
        for (uint32_t s = 0; s + 1 < PER; ++s) {
            v[r][0][s] = lo[r] + s < c0[r] ? lcp[lo[r] + s] : TOP;
            v[r][1][s] = c1[r] + s < hi[r] ? lcp[c1[r] + s] : TOP;
        }
    }
    for (uint64_t k = 0; c0[0] + k < c1[0] || c0[1] + k < c1[1]; k += (uint64_t)U * PER) {
        KmerChunk<idx_t> ch[2][U];
        UNROLL
        for (uint32_t r = 0; r < 2; ++r) {
            UNROLL
            for (uint32_t u = 0; u < U; ++u) {
                const uint64_t at = c0[r] + k + (uint64_t)u * PER;
                if (at < c1[r]) {
                    ch[r][u] = *reinterpret_cast<const KmerChunk<idx_t>*>(lcp + at);
                } else {
                    UNROLL
                    for (uint32_t j = 0; j < PER; ++j) ch[r][u].v[j] = TOP;
                }
            }
        }
        UNROLL
        for (uint32_t r = 0; r < 2; ++r) {
            UNROLL
            for (uint32_t u = 0; u < U; ++u) {
                UNROLL
                for (uint32_t j = 0; j < PER; ++j) m = ch[r][u].v[j] < m ? ch[r][u].v[j] : m;
            }
        }
    }
    UNROLL
    for (uint32_t r = 0; r < 2; ++r) {
        UNROLL
        for (uint32_t s = 0; s + 1 < PER; ++s) {
            m = v[r][0][s] < m ? v[r][0][s] : m;
            m = v[r][1][s] < m ? v[r][1][s] : m;
        }
    }
    return m;
}
// `cnt` entries from `first` (1 <= cnt, first + cnt <= size) of the table tier at base are covered by the first and the last 2^level
// entries of the run, level = floor(log2 cnt): the table of that level and the two indices.  Level and indices are clamped to the
// tier, whatever the arguments.
template <typename idx_t>
DEV_INLINE void lce_cover(const char* __restrict__ base, uint64_t stride, uint32_t levels, uint64_t size, uint64_t first, uint64_t cnt,
                          const idx_t*& tab, uint64_t& x, uint64_t& y)
{
    uint32_t j = 63u - (uint32_t)caps_clz64(cnt | 1);
    j = j < levels ? j : levels - 1;
    tab = reinterpret_cast<const idx_t*>(base + (uint64_t)j * stride);
    const uint64_t w = (uint64_t)1 << j;
    x = first;
    y = first + cnt - (cnt < w ? cnt : w);
    x = x < size ? x : size - 1;
    y = y < size ? y : size - 1;
}
// range_min(lo, hi), lo <= hi < v.n.  The (up to six) table reads are issued first, so that they are in flight during the scans.
template <typename idx_t>
DEV_INLINE idx_t lce_range_min(const LceView& v, uint64_t lo, uint64_t hi)
{
    constexpr idx_t TOP = (idx_t)~(idx_t)0;
    const idx_t* __restrict__ lcp = reinterpret_cast<const idx_t*>(v.lcp);
    const uint64_t bl = lo / LCE_BLOCK, bh = hi / LCE_BLOCK;
    const bool head_whole = lo % LCE_BLOCK == 0, tail_whole = hi % LCE_BLOCK == LCE_BLOCK - 1 || hi == v.n - 1;
    if (bl == bh && !(head_whole && tail_whole)) return lce_scan2<idx_t>(lcp, lo, hi + 1, 0, 0, TOP);
    const uint64_t fb = head_whole ? bl : bl + 1, le = tail_whole ? bh + 1 : bh;    // the whole blocks fb .. le - 1
    const uint64_t cnt = le > fb ? le - fb : 0;
    // three runs: blocks (all of them if at most 64, else those up to the next superblock edge), blocks from the last edge, superblocks
    uint64_t e1 = (fb + LCE_BPS - 1) / LCE_BPS * LCE_BPS, e2 = le / LCE_BPS * LCE_BPS;   // superblock edges, e1 <= e2 where cnt > 64
    const bool small = cnt <= LCE_BPS;
    const uint64_t cA = small ? cnt : e1 - fb, cB = small ? 0 : le - e2, cC = small ? 0 : (e2 - e1) / LCE_BPS;
    const idx_t* tA = nullptr;
    const idx_t* tB = nullptr;
    const idx_t* tC = nullptr;
    uint64_t xA = 0, yA = 0, xB = 0, yB = 0, xC = 0, yC = 0;
    idx_t r0 = TOP, r1 = TOP, r2 = TOP, r3 = TOP, r4 = TOP, r5 = TOP;
    if (cA) { lce_cover<idx_t>(v.m, v.m_stride, LCE_MLEVELS, v.nb, fb, cA, tA, xA, yA); r0 = tA[xA]; r1 = tA[yA]; }
    if (cB) { lce_cover<idx_t>(v.m, v.m_stride, LCE_MLEVELS, v.nb, e2, cB, tB, xB, yB); r2 = tB[xB]; r3 = tB[yB]; }
    if (cC) { lce_cover<idx_t>(v.t, v.t_stride, v.tlevels, v.ns, e1 / LCE_BPS, cC, tC, xC, yC); r4 = tC[xC]; r5 = tC[yC]; }
    idx_t m = lce_scan2<idx_t>(lcp, lo, head_whole ? lo : (bl + 1) * LCE_BLOCK, bh * LCE_BLOCK, tail_whole ? bh * LCE_BLOCK : hi + 1, TOP);
    m = r0 < m ? r0 : m;
    m = r1 < m ? r1 : m;
    m = r2 < m ? r2 : m;
    m = r3 < m ? r3 : m;
    m = r4 < m ? r4 : m;
    return r5 < m ? r5 : m;
}

// out[x] = range_min(lo[x], hi[x]); lo > hi or hi >= n: 0 and bit 0 of *flags
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) lce_range_min_kernel(KCTX LceView v, const uint64_t* __restrict__ lo, const uint64_t* __restrict__ hi, uint64_t q,
                                                     uint64_t* __restrict__ out, uint32_t* __restrict__ flags)
{
    PAR(tid) {
        for (uint64_t x = (uint64_t)K_BLOCK_IDX * FM_NT + tid; x < q; x += (uint64_t)K_GRID_DIM * FM_NT) {
            const uint64_t a = lo[x], b = hi[x];
            if (a > b || b >= v.n) {
                out[x] = 0;
                ATOMIC_OR_U32(flags, 1u);
                continue;
            }
            out[x] = (uint64_t)lce_range_min<idx_t>(v, a, b);
        }
    }
}

// out[x] = lce(I[x], J[x], k) by kangaroo jumps: at most k + 1 rounds of two ISA reads and one range minimum.  A position >= n: 0 and
// bit 0 of *flags.  Two equal ranks (no permutation) extend by 0.
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) lce_query_kernel(KCTX LceView v, const uint64_t* __restrict__ I, const uint64_t* __restrict__ J, uint64_t q,
                                                 uint32_t k, uint64_t* __restrict__ out, uint32_t* __restrict__ flags)
{
    const idx_t* __restrict__ isa = reinterpret_cast<const idx_t*>(v.isa);
    PAR(tid) {
        for (uint64_t x = (uint64_t)K_BLOCK_IDX * FM_NT + tid; x < q; x += (uint64_t)K_GRID_DIM * FM_NT) {
            const uint64_t i = I[x], j = J[x];
            if (i >= v.n || j >= v.n) {
                out[x] = 0;
                ATOMIC_OR_U32(flags, 1u);
                continue;
            }
            const uint64_t room = v.n - (i > j ? i : j);                             // no extension is longer
            uint64_t l = room;
            if (i != j) {
                l = 0;
                for (uint32_t used = 0;; ++used) {
                    uint64_t a = (uint64_t)isa[i + l], b = (uint64_t)isa[j + l];
                    a = a < v.n ? a : v.n - 1;
                    b = b < v.n ? b : v.n - 1;
                    uint64_t e = 0;
                    if (a != b) e = (uint64_t)lce_range_min<idx_t>(v, (a < b ? a : b) + 1, a < b ? b : a);
                    l += e < room - l ? e : room - l;
                    if (l == room || used == k) break;
                    ++l;                                                             // the mismatch
                    if (l == room) break;
                }
            }
            out[x] = l;
        }
    }
}

// ---- MUMs and rare MEMs between two texts (capi_impl.h cross_*; include/caps_sa_hip.h "MUMs and MEMs between two texts") ----------------
// T = A . sep . B, side(p) = (p >= split).  Every decision is a rule over neighbouring ranks of (SA, LCP, BWT); nothing is indexed by a
// value read from SA or LCP.  Tiles of XM_TILE ranks, FM_NT threads, grid-stride, count -> fm_scan_kernel -> write as the k-mer table:
//   xm_kernel<COUNT>   coalesced 16-byte loads of LCP; SA and BWT only for a chunk with a rank that can yield a record (LCP >= min_len)
//                      or beat the thread's longest-common-substring candidate; the neighbours across a chunk or tile edge are read
//                      from global memory.  Leaves cnt[tile] (records), cnt[n_tiles + tile] (skipped runs, counted at their heads)
//                      and per workgroup its LCS candidate (length, rank; a thread meets its ranks in ascending order).
//   xm_kernel<WRITE>   repeats the decisions, leaves every rank's number of records as a byte in LDS; then a lane owns XM_LANE
//                      consecutive ranks, the lanes' sums are scanned (kmer_run_kernel's two steps) and the records stored in rank order.
//   xm_finish_kernel   one workgroup: the lowest rank among the longest candidates, the 8 summary words.
// MEM mode (MEMS, max_occ >= 2): rank q with LCP[q] >= min_len walks back over at most max_occ - 1 ranks to its run's head and
// forward to its end: at most max_occ + 1 reads of LCP and max_occ - 1 of SA and of BWT per rank, whatever the arrays hold.
constexpr uint64_t XM_TILE = KMER_TILE;
constexpr uint32_t XM_LANE = KMER_LANE;
constexpr uint32_t XM_MAX_OCC = 64;
constexpr uint32_t XM_KEYS = 2;                                    // columns of the tile counts: records, skipped runs
enum { XM_COUNT = 0, XM_WRITE = 1 };
static_assert(KmerGeom<uint32_t>::ROUNDS % 4 == 0 && KmerGeom<uint64_t>::ROUNDS % 4 == 0 && XM_MAX_OCC - 1 <= 255 && XM_LANE * (XM_MAX_OCC - 1) < (1u << 16), "a rank's records fit a byte, a tile's 32 bits");
template <typename idx_t> struct XmIn {
    const idx_t* SA;
    const idx_t* LCP;
    const uint8_t* BWT;
    uint64_t n, split, min_len;
    uint32_t max_occ;
};

// rank q (1 <= q < n, LCP[q] >= min_len) of MEM mode: its pairs (p, q), p descending -> f(SA[p], SA[q], min LCP[p + 1 .. q]).  CHECK:
// returns their number, 0 for a run that is given up (no head within max_occ - 1 ranks below q, or no end within max_occ ranks of the head);
// without CHECK the caller knows that the run is processed.
template <typename idx_t, bool CHECK, typename F>
DEV_INLINE uint32_t xm_mem_rank(const XmIn<idx_t>& a, uint64_t q, F&& f)
{
    const uint64_t sq = (uint64_t)a.SA[q];
    const uint32_t bq = a.BWT[q];
    uint64_t l = (uint64_t)a.LCP[q], h = q;
    uint32_t found = 0;
    bool head = false;
    for (uint32_t d = 1; d < a.max_occ; ++d) {
        const uint64_t p = q - d, sp = (uint64_t)a.SA[p];
        if ((sp >= a.split) != (sq >= a.split) && (sp == 0 || sq == 0 || (uint32_t)a.BWT[p] != bq)) { f(sp, sq, l); ++found; }
        if (p == 0) { h = 0; head = true; break; }
        const uint64_t lp = (uint64_t)a.LCP[p];
        if (lp < a.min_len) { h = p; head = true; break; }
        l = lp < l ? lp : l;
    }
    if (!CHECK) return found;
    if (!head) return 0;
    for (uint64_t e = q + 1; e <= h + a.max_occ; ++e)
        if (e >= a.n || (uint64_t)a.LCP[e] < a.min_len) return found;
    return 0;
}
// head h of MEM mode: is its run longer than max_occ ranks?
template <typename idx_t>
DEV_INLINE bool xm_run_skipped(const XmIn<idx_t>& a, uint64_t h)
{
    for (uint64_t e = h + 1; e <= h + a.max_occ; ++e)
        if (e >= a.n || (uint64_t)a.LCP[e] < a.min_len) return false;
    return true;
}
HD void xm_store(uint64_t* __restrict__ rec, uint64_t at, uint64_t cap, uint64_t sp, uint64_t sq, uint64_t l, uint64_t split)
{
    if (at < cap) {
        rec[3 * at] = sp < split ? sp : sq;
        rec[3 * at + 1] = sp < split ? sq : sp;
        rec[3 * at + 2] = l;
    }
}

template <typename idx_t, int MODE, bool MEMS>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) xm_kernel(KCTX const idx_t* __restrict__ SA, const idx_t* __restrict__ LCP, const uint8_t* __restrict__ BWT, uint64_t n,
                                          uint64_t split, uint64_t min_len, uint32_t max_occ, uint64_t n_tiles, uint64_t* __restrict__ cnt,
                                          uint64_t* __restrict__ lcs, uint64_t* __restrict__ rec, uint64_t cap)
{
    using G = KmerGeom<idx_t>;
    constexpr uint32_t PER = G::PER;
    SHARED_ARRAY(uint8_t, rc, MODE == XM_WRITE ? XM_TILE : 1);      // per rank: its records
    SHARED_ARRAY(uint32_t, lane, FM_NT);
    SHARED_ARRAY(uint32_t, scan, FM_NT);
    SHARED_ARRAY(uint32_t, grp, 2 * KMER_GROUP);
    SHARED_ARRAY(uint32_t, h, XM_KEYS);
    SHARED_ARRAY(uint64_t, bl, MODE == XM_COUNT ? FM_NT : 1);
    SHARED_ARRAY(uint64_t, br, MODE == XM_COUNT ? FM_NT : 1);
    TL_DECL(uint64_t, best, 2);                                     // the thread's LCS candidate: length, rank
    const XmIn<idx_t> a{SA, LCP, BWT, n, split, min_len, max_occ};
    constexpr bool mems = MEMS;                                     // (MUM mode: max_occ = 0)
    PAR(tid) {
        TL(best, tid, 0) = 0;
        TL(best, tid, 1) = 0;
        if (tid < XM_KEYS) h[tid] = 0;
    }
    SYNC();
    for (uint64_t tile = K_BLOCK_IDX; tile < n_tiles; tile += K_GRID_DIM) {         // block-uniform
        const uint64_t t0 = tile * XM_TILE;
        PAR(tid) {
            uint32_t mine = 0, skipped = 0;
            uint64_t bestl = TL(best, tid, 0), bestr = TL(best, tid, 1);
            // four chunks of LCP in flight (with the rank before and the rank behind each: the neighbours' cache lines), then the decisions
            for (uint32_t j0 = 0; j0 < G::ROUNDS; j0 += 4) {
                KmerChunk<idx_t> lc4[4];
                idx_t bef4[4], beh4[4];
                UNROLL
                for (uint32_t j = 0; j < 4; ++j) {
                    const uint64_t i0 = t0 + (uint64_t)((j0 + j) * FM_NT + tid) * PER;
                    bef4[j] = beh4[j] = 0;
                    if (i0 < n) {
                        lc4[j] = kmer_load<idx_t>(LCP, n, i0);
                        if (i0 >= 2) bef4[j] = LCP[i0 - 1];
                        if (i0 + PER < n) beh4[j] = LCP[i0 + PER];
                    }
                }
                UNROLL
                for (uint32_t j = 0; j < 4; ++j) {
                    const uint32_t c = (j0 + j) * FM_NT + tid;
                    const uint64_t i0 = t0 + (uint64_t)c * PER;
                    uint32_t made[PER];
                    UNROLL
                    for (uint32_t e = 0; e < PER; ++e) made[e] = 0;
                    if (i0 < n) {
                        // eff[1 + e] = LCP[i0 + e] as the rules see it: 0 at rank 0 and behind the last rank
                        const KmerChunk<idx_t>& lc = lc4[j];
                        uint64_t eff[PER + 2];
                        eff[0] = (uint64_t)bef4[j];
                        UNROLL
                        for (uint32_t e = 0; e < PER; ++e) eff[1 + e] = (uint64_t)lc.v[e];
                        if (i0 == 0) eff[1] = 0;
                        eff[PER + 1] = (uint64_t)beh4[j];
                        bool want = false;
                        UNROLL
                        for (uint32_t e = 0; e < PER; ++e) {
                            const uint64_t l = eff[1 + e];
                            bool w = l >= min_len && (mems || (eff[e] < l && eff[2 + e] < l));
                            if (MODE == XM_COUNT) w = w || l > bestl;
                            want = want || w;
                        }
                        if (want) {                                    // (a rank with l >= 1 is at least 1 and below n)
                            const KmerChunk<idx_t> sc = kmer_load<idx_t>(SA, n, i0);
                            const uint64_t before = i0 ? (uint64_t)SA[i0 - 1] : 0;
                            UNROLL
                            for (uint32_t e = 0; e < PER; ++e) {
                                const uint64_t l = eff[1 + e], r = i0 + e;
                                if (l == 0) continue;
                                const uint64_t sp = e ? (uint64_t)sc.v[e ? e - 1 : 0] : before, sq = (uint64_t)sc.v[e];
                                const bool crossing = (sp >= split) != (sq >= split);
                                if (MODE == XM_COUNT && crossing && l > bestl) { bestl = l; bestr = r; }
                                if (l < min_len) continue;
                                if (mems) made[e] = xm_mem_rank<idx_t, true>(a, r, [](uint64_t, uint64_t, uint64_t) {});
                                else if (crossing && eff[e] < l && eff[2 + e] < l && (sp == 0 || sq == 0 || BWT[r - 1] != BWT[r])) made[e] = 1;
                            }
                        }
                        if (MODE == XM_COUNT && mems) {                 // the heads of the chunk whose next rank is none: runs of 2 ranks or more
                            UNROLL
                            for (uint32_t e = 0; e < PER; ++e)
                                if (i0 + e < n && eff[1 + e] < min_len && eff[2 + e] >= min_len && xm_run_skipped<idx_t>(a, i0 + e)) ++skipped;
                        }
                    }
                    UNROLL
                    for (uint32_t e = 0; e < PER; ++e) {
                        mine += made[e];
                        if (MODE == XM_WRITE) rc[c * PER + e] = (uint8_t)made[e];
                    }
                }
            }
            if (MODE == XM_COUNT) {
                TL(best, tid, 0) = bestl;
                TL(best, tid, 1) = bestr;
                if (mine) FETCH_ADD_U32(&h[0], mine);
                if (skipped) FETCH_ADD_U32(&h[1], skipped);
            }
        }
        SYNC();
        if (MODE == XM_COUNT) {
            PAR(tid) {
                if (tid < XM_KEYS) {
                    cnt[(uint64_t)tid * n_tiles + tile] = h[tid];
                    h[tid] = 0;
                }
            }
            SYNC();
        }
        if (MODE == XM_WRITE) {
            PAR(tid) {
                uint32_t s = 0;
                for (uint32_t k = 0; k < XM_LANE; ++k) s += rc[tid * XM_LANE + k];
                lane[tid] = s;
            }
            SYNC();
            PAR(tid) {                                      // forward: the records of the lanes before every lane
                if (tid < KMER_GROUP) {
                    uint32_t run = 0;
                    for (uint32_t j = 0; j < KMER_GROUP; ++j) {
                        const uint32_t at = tid * KMER_GROUP + j, x = lane[at];
                        scan[at] = run;
                        run += x;
                    }
                    grp[tid] = run;
                }
            }
            SYNC();
            PAR(tid) {
                if (tid == 0) {
                    uint32_t run = 0;
                    for (uint32_t g = 0; g < KMER_GROUP; ++g) { const uint32_t x = grp[g]; grp[KMER_GROUP + g] = run; run += x; }
                }
            }
            SYNC();
            PAR(tid) {
                if (lane[tid]) {
                    uint64_t at = cnt[tile] + scan[tid] + grp[KMER_GROUP + tid / KMER_GROUP];
                    for (uint32_t k = 0; k < XM_LANE; ++k) {
                        if (!rc[tid * XM_LANE + k]) continue;
                        const uint64_t r = t0 + (uint64_t)tid * XM_LANE + k;         // 1 <= r < n: it made records
                        if (mems) {
                            xm_mem_rank<idx_t, false>(a, r, [&](uint64_t sp, uint64_t sq, uint64_t l) { xm_store(rec, at, cap, sp, sq, l, split); ++at; });
                        } else {
                            xm_store(rec, at, cap, (uint64_t)SA[r - 1], (uint64_t)SA[r], (uint64_t)LCP[r], split);
                            ++at;
                        }
                    }
                }
            }
            SYNC();
        }
    }
    if (MODE == XM_COUNT) {
        PAR(tid) {
            bl[tid] = TL(best, tid, 0);
            br[tid] = TL(best, tid, 1);
        }
        SYNC();
        PAR(tid) {
            if (tid == 0) {
                uint64_t l = 0, r = 0;
                for (uint32_t k = 0; k < FM_NT; ++k)
                    if (bl[k] > l || (bl[k] == l && l && br[k] < r)) { l = bl[k]; r = br[k]; }
                lcs[2 * (uint64_t)K_BLOCK_IDX] = l;
                lcs[2 * (uint64_t)K_BLOCK_IDX + 1] = r;
            }
        }
    }
}

// one workgroup: out[0] = records, out[1] = skipped runs (tot[] of fm_scan_kernel), out[2 .. 4] = the LCS (len, a, b) from the lowest rank
// among the workgroups' longest candidates (a candidate rank r has 1 <= r < n), out[5 .. 7] = 0
template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) xm_finish_kernel(KCTX const idx_t* __restrict__ SA, uint64_t n, uint64_t split, const uint64_t* __restrict__ lcs,
                                                 uint32_t groups, const uint64_t* __restrict__ tot, uint64_t* __restrict__ out)
{
    SHARED_ARRAY(uint64_t, bl, FM_NT);
    SHARED_ARRAY(uint64_t, br, FM_NT);
    PAR(tid) {
        uint64_t l = 0, r = 0;
        for (uint32_t g = tid; g < groups; g += FM_NT) {
            const uint64_t gl = lcs[2 * (uint64_t)g], gr = lcs[2 * (uint64_t)g + 1];
            if (gl > l || (gl == l && l && gr < r)) { l = gl; r = gr; }
        }
        bl[tid] = l;
        br[tid] = r;
    }
    SYNC();
    PAR(tid) {
        if (tid == 0) {
            uint64_t l = 0, r = 0;
            for (uint32_t k = 0; k < FM_NT; ++k)
                if (bl[k] > l || (bl[k] == l && l && br[k] < r)) { l = bl[k]; r = br[k]; }
            out[0] = tot[0];
            out[1] = tot[1];
            out[2] = out[3] = out[4] = out[5] = out[6] = out[7] = 0;
            if (l && r >= 1 && r < n) {
                const uint64_t sp = (uint64_t)SA[r - 1], sq = (uint64_t)SA[r];
                out[2] = l;
                out[3] = sp < split ? sp : sq;
                out[4] = sp < split ? sq : sp;
            }
        }
    }
}

// ---- k-mers across a collection (capi_impl.h coll_*; include/caps_sa_hip.h "k-mers across a collection") ------------------------------
// Heads and runs are kmer_*'s; every rank of a run that lies IN a document adds that document's bit to the run's `docs` and 1 to its
// `occ`: a segmented OR and a segmented sum whose segments are the runs.  Tiles of KMER_TILE ranks, FM_NT threads, grid-stride:
//   ck_edge_kernel   per tile: its first head (n: none), and (docs, occ) of the ranks in front of it -- the part of the tile that belongs
//                    to a run headed in an earlier tile.  LCP is read up to the first head, SA only in front of it.
//   ck_close_kernel  one workgroup, backward over the tiles: carry[t] = what the tiles behind t add to the run that is open at t's end
//                    (over any number of headless tiles, up to and with the front part of the next tile that has a head)
//   kmer_next_kernel next[t] = the first head at or after tile t (run lengths across tiles)
//   ck_run_kernel    per tile: coalesced 16-byte loads of LCP and SA leave one byte per rank in LDS (its document, CK_OUT, CK_HEAD); a
//                    lane owns KMER_LANE consecutive ranks; the lanes' front parts are scanned backward in two steps of 16 as
//                    (docs, occ, has a head), then every lane closes the runs it heads.  No lane walks beyond its own 64 ranks.
// The document of a position is the result of at most 6 comparisons with the table in LDS; nothing is indexed by a value read from SA
// or LCP.
constexpr uint32_t CK_MAX_DOCS = 64;
constexpr uint32_t CK_OUT = 0x40u, CK_HEAD = 0x80u;                // bits of a rank's byte; bits 0 .. 5: its document
constexpr uint32_t CK_NONE = 0xFFFFFFFFu;
constexpr uint32_t CK_LANE_WORDS = KMER_LANE / 4;                  // a lane's bytes as words ...
constexpr uint32_t CK_LANE_PITCH = CK_LANE_WORDS + 1;              // ... one word apart: lanes that read word j hit different banks
constexpr uint32_t CK_CELLS = CK_MAX_DOCS * CK_MAX_DOCS;           // the matrix, cell [a][b] with a <= b
constexpr uint32_t CK_FREQ = CK_CELLS;                             // then freq[0 .. 64]
constexpr uint32_t CK_FULL = CK_FREQ + CK_MAX_DOCS + 1;            // then the k-mers that every document has
constexpr uint32_t CK_COLS = CK_FULL + 1;
#ifdef CAPS_EMUL
constexpr uint32_t CK_FLUSH_TILES = 2;                             // small on purpose: the flush runs
#else
constexpr uint32_t CK_FLUSH_TILES = 1u << 16;                      // a tile adds at most 2^14 to a 32-bit counter of its workgroup
#endif
enum { CK_COUNT = 0, CK_WRITE = 1, CK_SHARING = 2 };
struct CkFilter { uint64_t min_docs, max_docs, all_of, none_of; };

// the table in LDS: start[64] | end[64]; entries from m on hold start = 2^64 - 1, end = 0
DEV_INLINE void ck_load_table(uint64_t* __restrict__ tab, const uint64_t* __restrict__ dtab, uint32_t tid)
{
    for (uint32_t j = tid; j < 2 * CK_MAX_DOCS; j += FM_NT) tab[j] = dtab[j];
}
// the document that holds p .. p + k - 1, or CK_OUT; top = the power of two >= m
DEV_INLINE uint32_t ck_doc(const uint64_t* __restrict__ tab, uint32_t top, uint64_t p, uint64_t k)
{
    uint32_t d = 0;
    for (uint32_t step = top >> 1; step; step >>= 1) d += tab[d + step] <= p ? step : 0u;
    const uint64_t s = tab[d], e = tab[CK_MAX_DOCS + d];
    return s <= p && p <= e && e - p >= k ? d : CK_OUT;
}

template <typename idx_t>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) ck_edge_kernel(KCTX const idx_t* __restrict__ SA, const idx_t* __restrict__ LCP, uint64_t n, uint64_t k,
                                               uint64_t n_tiles, const uint64_t* __restrict__ dtab, uint32_t top, uint64_t* __restrict__ head,
                                               uint64_t* __restrict__ pd, uint64_t* __restrict__ po)
{
    using G = KmerGeom<idx_t>;
    SHARED_ARRAY(uint64_t, tab, 2 * CK_MAX_DOCS);
    SHARED_ARRAY(uint32_t, acc, 4);                        // the first head (tile-relative), docs low / high, occ
    PAR(tid) { ck_load_table(tab, dtab, tid); }
    SYNC();
    for (uint64_t tile = K_BLOCK_IDX; tile < n_tiles; tile += K_GRID_DIM) {         // block-uniform
        const uint64_t t0 = tile * KMER_TILE;
        PAR(tid) { if (tid < 4) acc[tid] = tid == 0 ? (uint32_t)KMER_TILE : 0u; }
        SYNC();
        PAR(tid) {                                          // kmer_head_kernel's search: a lane stops at its first head
            uint32_t best = (uint32_t)KMER_TILE;
            for (uint32_t j0 = 0; j0 < G::ROUNDS && best == (uint32_t)KMER_TILE; j0 += 4) {
                uint32_t hb[4];
                UNROLL
                for (uint32_t j = 0; j < 4; ++j) {
                    const uint64_t i0 = t0 + (uint64_t)((j0 + j) * FM_NT + tid) * G::PER;
                    hb[j] = i0 < n ? kmer_head_bits<idx_t>(LCP, n, k, i0) : 0u;
                }
                UNROLL
                for (uint32_t j = 0; j < 4; ++j)
                    if (hb[j] && best == (uint32_t)KMER_TILE) best = ((j0 + j) * FM_NT + tid) * G::PER + (uint32_t)__builtin_ctz(hb[j]);
            }
            if (best < (uint32_t)KMER_TILE) ATOMIC_MIN_U32(&acc[0], best);
        }
        SYNC();
        PAR(tid) {                                          // the ranks in front of it
            const uint64_t lim = std::min<uint64_t>(acc[0], n - t0);
            uint64_t docs = 0;
            uint32_t occ = 0;
            for (uint32_t c = tid; (uint64_t)c * G::PER < lim; c += FM_NT) {
                const uint64_t i0 = t0 + (uint64_t)c * G::PER;
                const KmerChunk<idx_t> s = kmer_load<idx_t>(SA, n, i0);
                UNROLL
                for (uint32_t e = 0; e < G::PER; ++e) {
                    const uint32_t d = ck_doc(tab, top, (uint64_t)s.v[e], k);
                    if ((uint64_t)c * G::PER + e < lim && d != CK_OUT) { docs |= 1ull << d; ++occ; }
                }
            }
            if ((uint32_t)docs) ATOMIC_OR_U32(&acc[1], (uint32_t)docs);
            if ((uint32_t)(docs >> 32)) ATOMIC_OR_U32(&acc[2], (uint32_t)(docs >> 32));
            if (occ) FETCH_ADD_U32(&acc[3], occ);
        }
        SYNC();
        PAR(tid) {
            if (tid == 0) {
                head[tile] = acc[0] < (uint32_t)KMER_TILE ? t0 + acc[0] : n;
                pd[tile] = (uint64_t)acc[1] | ((uint64_t)acc[2] << 32);
                po[tile] = acc[3];
            }
        }
        SYNC();
    }
}

// one workgroup, kmer_next_kernel's shape with the segmented (OR, sum) from the right: S[t] = front[t] if tile t has a head, else
// front[t] + S[t + 1]; cd / co[t] = S[t + 1], S[n_tiles] = nothing.  head[] is ck_edge_kernel's (n: no head), not yet kmer_next_kernel's.
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) ck_close_kernel(KCTX const uint64_t* __restrict__ head, const uint64_t* __restrict__ pd,
                                                const uint64_t* __restrict__ po, uint64_t* __restrict__ cd, uint64_t* __restrict__ co,
                                                uint64_t n_tiles, uint64_t n)
{
    SHARED_ARRAY(uint64_t, part_d, FM_NT);
    SHARED_ARRAY(uint64_t, part_o, FM_NT);
    SHARED_ARRAY(uint32_t, part_f, FM_NT);
    const uint64_t per = (n_tiles + FM_NT - 1) / FM_NT;
    PAR(tid) {
        const uint64_t a = std::min<uint64_t>(n_tiles, tid * per), b = std::min<uint64_t>(n_tiles, a + per);
        uint64_t d = 0, o = 0;
        uint32_t f = 0;
        for (uint64_t t = b; t-- > a;) {
            if (head[t] < n) { d = pd[t]; o = po[t]; f = 1; }
            else { d |= pd[t]; o += po[t]; }
        }
        part_d[tid] = d;
        part_o[tid] = o;
        part_f[tid] = f;
    }
    SYNC();
    PAR(tid) {
        if (tid == 0) {
            uint64_t d = 0, o = 0;
            for (uint32_t t = FM_NT; t-- > 0;) {
                const uint64_t vd = part_d[t], vo = part_o[t];
                part_d[t] = d;
                part_o[t] = o;
                if (part_f[t]) { d = vd; o = vo; }
                else { d |= vd; o += vo; }
            }
        }
    }
    SYNC();
    PAR(tid) {
        const uint64_t a = std::min<uint64_t>(n_tiles, tid * per), b = std::min<uint64_t>(n_tiles, a + per);
        uint64_t d = part_d[tid], o = part_o[tid];
        for (uint64_t t = b; t-- > a;) {
            cd[t] = d;
            co[t] = o;
            if (head[t] < n) { d = pd[t]; o = po[t]; }
            else { d |= pd[t]; o += po[t]; }
        }
    }
}

// a lane's bytes: (docs, occ) of the ranks in front of its first head, and that head (lane-relative; CK_NONE: no head, all of the lane)
DEV_INLINE void ck_front(const uint32_t* __restrict__ w16, uint64_t& docs, uint32_t& occ, uint32_t& first)
{
    docs = 0;
    occ = 0;
    first = CK_NONE;
    for (uint32_t j = 0; j < CK_LANE_WORDS && first == CK_NONE; ++j) {
        const uint32_t w = w16[j];
        UNROLL
        for (uint32_t e = 0; e < 4; ++e) {
            const uint32_t b = (w >> (8 * e)) & 0xFFu;
            if ((b & CK_HEAD) && first == CK_NONE) first = 4 * j + e;
            if (first == CK_NONE && !(b & CK_OUT)) { docs |= 1ull << (b & 63u); ++occ; }
        }
    }
}
// the runs a lane heads, in rank order: f(head rank, count, occ, docs) for those with docs != 0.  Behind the lane's last head the run goes
// on to lane_next and gains (tail_d, tail_o).  A lane behind the last rank heads nothing.
template <typename F>
DEV_INLINE void ck_each_run(const uint32_t* __restrict__ w16, uint64_t r0, uint64_t n, uint64_t tail_d, uint64_t tail_o, uint64_t lane_next, F&& f)
{
    if (r0 >= n) return;
    uint64_t docs = 0;
    uint32_t occ = 0, hd = CK_NONE;
    for (uint32_t j = 0; j < CK_LANE_WORDS; ++j) {
        const uint32_t w = w16[j];
        UNROLL
        for (uint32_t e = 0; e < 4; ++e) {
            const uint32_t b = (w >> (8 * e)) & 0xFFu, p = 4 * j + e;
            if (b & CK_HEAD) {
                if (hd != CK_NONE && docs) f(r0 + hd, (uint64_t)(p - hd), (uint64_t)occ, docs);
                hd = p;
                docs = 0;
                occ = 0;
            }
            if (!(b & CK_OUT)) { docs |= 1ull << (b & 63u); ++occ; }
        }
    }
    if (hd != CK_NONE) {
        docs |= tail_d;
        if (docs) f(r0 + hd, lane_next - (r0 + hd), (uint64_t)occ + tail_o, docs);
    }
}
HD bool ck_passes(const CkFilter& q, uint64_t docs)
{
    const uint64_t c = (uint64_t)__builtin_popcountll(docs);
    return c >= q.min_docs && (q.max_docs == 0 || c <= q.max_docs) && (docs & q.all_of) == q.all_of && (docs & q.none_of) == 0;
}

// MODE CK_COUNT:   cnt[tile] = the collection k-mers headed in the tile that pass the filter.
// MODE CK_WRITE:   cnt[] scanned (fm_scan_kernel); the same k-mers as records (first | count | occ | docs) at cnt[tile] + their number in
//                  the tile, four 8-byte stores each; a slot at or beyond cap is not written.
// MODE CK_SHARING: every collection k-mer into the workgroup's counters in LDS -- a k-mer of all m documents into a register (added to
//                  every cell on the host), one of a single document with one atomic on its diagonal cell and a register for freq[1],
//                  any other by its owning lane, one atomic per pair a <= b of its bits.  The counters go out to
//                  hist[workgroup * CK_COLS + column] as 64-bit sums, every CK_FLUSH_TILES tiles of the workgroup and at its end.
template <typename idx_t, int MODE>
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) ck_run_kernel(KCTX const idx_t* __restrict__ SA, const idx_t* __restrict__ LCP, uint64_t n, uint64_t k,
                                              uint64_t n_tiles, const uint64_t* __restrict__ dtab, uint32_t top, uint32_t m,
                                              const uint64_t* __restrict__ next, const uint64_t* __restrict__ cd,
                                              const uint64_t* __restrict__ co, CkFilter q, uint64_t* __restrict__ cnt,
                                              uint64_t* __restrict__ rec, uint64_t cap, uint64_t* __restrict__ hist)
{
    using G = KmerGeom<idx_t>;
    SHARED_ARRAY(uint64_t, tab, 2 * CK_MAX_DOCS);
    SHARED_ARRAY(uint32_t, rk, FM_NT * CK_LANE_PITCH);     // a byte per rank, a lane's 16 words CK_LANE_PITCH apart
    SHARED_ARRAY(uint64_t, xd, FM_NT);                     // per lane: the docs in front of its first head
    SHARED_ARRAY(uint32_t, xo, FM_NT);                     // ... and their occurrences
    SHARED_ARRAY(uint32_t, lane, FM_NT);                   // per lane: its first head (tile-relative; KMER_TILE: none), then its records
    SHARED_ARRAY(uint32_t, scan, FM_NT);                   // the scan of lane[] inside its group of 16, exclusive
    SHARED_ARRAY(uint64_t, rd, FM_NT);                     // what the lanes behind add to a lane's open run, inside its group
    SHARED_ARRAY(uint32_t, ro, FM_NT);
    SHARED_ARRAY(uint32_t, grp, 2 * KMER_GROUP);           // per group: its min / sum, and the exclusive scan over the groups
    SHARED_ARRAY(uint64_t, gd, 2 * KMER_GROUP);
    SHARED_ARRAY(uint64_t, go, 2 * KMER_GROUP);
    SHARED_ARRAY(uint32_t, h, MODE == CK_SHARING ? CK_COLS : 1);
    TL_DECL(uint64_t, st, 3);                              // a lane's tail docs, tail occ, the first head behind its ranks
    TL_DECL(uint32_t, reg, 2);                             // CK_SHARING: the lane's k-mers of one document, of all m
    const uint64_t full = m < 64 ? (1ull << m) - 1 : ~0ull;
    uint32_t tiles_in = 0;                                 // block-uniform: tiles since the last flush
    bool flushed = false;
    PAR(tid) {
        ck_load_table(tab, dtab, tid);
        TL(reg, tid, 0) = 0;
        TL(reg, tid, 1) = 0;
        if (MODE == CK_SHARING) for (uint32_t b = tid; b < CK_COLS; b += FM_NT) h[b] = 0;
    }
    SYNC();
    for (uint64_t tile = K_BLOCK_IDX; tile < n_tiles; tile += K_GRID_DIM) {         // block-uniform
        const uint64_t t0 = tile * KMER_TILE;
        PAR(tid) {
            if (tid == 0 && MODE == CK_COUNT) h[0] = 0;
            UNROLL
            for (uint32_t j0 = 0; j0 < G::ROUNDS; j0 += 4) {
                uint32_t hb[4];
                KmerChunk<idx_t> s[4];
                UNROLL
                for (uint32_t j = 0; j < 4; ++j) {
                    const uint64_t i0 = t0 + (uint64_t)((j0 + j) * FM_NT + tid) * G::PER;
                    hb[j] = 0;
                    if (i0 < n) { hb[j] = kmer_head_bits<idx_t>(LCP, n, k, i0); s[j] = kmer_load<idx_t>(SA, n, i0); }
                    else for (uint32_t e = 0; e < G::PER; ++e) s[j].v[e] = 0;
                }
                UNROLL
                for (uint32_t j = 0; j < 4; ++j) {
                    const uint32_t c = (j0 + j) * FM_NT + tid;
                    const uint64_t i0 = t0 + (uint64_t)c * G::PER;
                    uint32_t w = 0;
                    UNROLL
                    for (uint32_t e = 0; e < G::PER; ++e) {
                        uint32_t b = CK_HEAD | CK_OUT;                               // a rank that does not exist ends the last run
                        if (i0 + e < n) b = ck_doc(tab, top, (uint64_t)s[j].v[e], k) | (((hb[j] >> e) & 1u) ? CK_HEAD : 0u);
                        w |= b << (8 * e);
                    }
                    const uint32_t ln = c * G::PER / KMER_LANE;
                    if (G::PER == 4) rk[c + ln] = w;
                    else reinterpret_cast<uint16_t*>(rk)[c + 2 * ln] = (uint16_t)w;
                }
            }
        }
        SYNC();
        PAR(tid) {
            uint64_t d;
            uint32_t o, first;
            ck_front(rk + tid * CK_LANE_PITCH, d, o, first);
            xd[tid] = d;
            xo[tid] = o;
            lane[tid] = first != CK_NONE ? tid * KMER_LANE + first : (uint32_t)KMER_TILE;
        }
        SYNC();
        PAR(tid) {                                          // backward: the first head behind every lane and what lies in front of it
            if (tid < KMER_GROUP) {
                uint32_t run = (uint32_t)KMER_TILE, so = 0;
                uint64_t sd = 0;
                for (uint32_t j = KMER_GROUP; j-- > 0;) {
                    const uint32_t at = tid * KMER_GROUP + j, x = lane[at];
                    scan[at] = run;
                    rd[at] = sd;
                    ro[at] = so;
                    if (x < (uint32_t)KMER_TILE) { sd = xd[at]; so = xo[at]; }
                    else { sd |= xd[at]; so += xo[at]; }
                    run = std::min(run, x);
                }
                grp[tid] = run;
                gd[tid] = sd;
                go[tid] = so;
            }
        }
        SYNC();
        PAR(tid) {
            if (tid == 0) {
                uint32_t run = (uint32_t)KMER_TILE;
                uint64_t sd = cd[tile], so = co[tile];
                for (uint32_t g = KMER_GROUP; g-- > 0;) {
                    const uint32_t x = grp[g];
                    grp[KMER_GROUP + g] = run;
                    gd[KMER_GROUP + g] = sd;
                    go[KMER_GROUP + g] = so;
                    if (x < (uint32_t)KMER_TILE) { sd = gd[g]; so = go[g]; }
                    else { sd |= gd[g]; so += go[g]; }
                    run = std::min(run, x);
                }
            }
        }
        SYNC();
        PAR(tid) {
            const uint32_t g = tid / KMER_GROUP;
            const uint32_t nx = std::min(scan[tid], grp[KMER_GROUP + g]);
            const uint64_t lane_next = nx < (uint32_t)KMER_TILE ? t0 + nx : next[tile + 1];
            uint64_t td = rd[tid], to = ro[tid];
            if (scan[tid] == (uint32_t)KMER_TILE) { td |= gd[KMER_GROUP + g]; to += go[KMER_GROUP + g]; }
            TL(st, tid, 0) = td;
            TL(st, tid, 1) = to;
            TL(st, tid, 2) = lane_next;
            const uint64_t r0 = t0 + (uint64_t)tid * KMER_LANE;
            if (MODE == CK_SHARING) {
                uint32_t one = 0, all = 0;
                ck_each_run(rk + tid * CK_LANE_PITCH, r0, n, td, to, lane_next, [&](uint64_t, uint64_t, uint64_t, uint64_t docs) {
                    if (docs == full) { ++all; return; }
                    if ((docs & (docs - 1)) == 0) {
                        const uint32_t a = (uint32_t)__builtin_ctzll(docs);
                        ++one;
                        FETCH_ADD_U32(&h[a * CK_MAX_DOCS + a], 1u);
                        return;
                    }
                    FETCH_ADD_U32(&h[CK_FREQ + (uint32_t)__builtin_popcountll(docs)], 1u);
                    for (uint64_t x = docs; x; x &= x - 1) {
                        const uint32_t a = (uint32_t)__builtin_ctzll(x);
                        for (uint64_t y = x; y; y &= y - 1) FETCH_ADD_U32(&h[a * CK_MAX_DOCS + (uint32_t)__builtin_ctzll(y)], 1u);
                    }
                });
                TL(reg, tid, 0) += one;
                TL(reg, tid, 1) += all;
            } else {
                uint32_t mine = 0;
                ck_each_run(rk + tid * CK_LANE_PITCH, r0, n, td, to, lane_next,
                            [&](uint64_t, uint64_t, uint64_t, uint64_t docs) { mine += ck_passes(q, docs) ? 1u : 0u; });
                if (MODE == CK_COUNT) { if (mine) FETCH_ADD_U32(&h[0], mine); }
                else lane[tid] = mine;
            }
        }
        SYNC();
        if (MODE == CK_COUNT) {
            PAR(tid) { if (tid == 0) cnt[tile] = h[0]; }
            SYNC();
        }
        if (MODE == CK_WRITE) {
            PAR(tid) {                                      // forward: the records of the lanes before every lane
                if (tid < KMER_GROUP) {
                    uint32_t run = 0;
                    for (uint32_t j = 0; j < KMER_GROUP; ++j) {
                        const uint32_t at = tid * KMER_GROUP + j, x = lane[at];
                        scan[at] = run;
                        run += x;
                    }
                    grp[tid] = run;
                }
            }
            SYNC();
            PAR(tid) {
                if (tid == 0) {
                    uint32_t run = 0;
                    for (uint32_t g = 0; g < KMER_GROUP; ++g) { const uint32_t x = grp[g]; grp[KMER_GROUP + g] = run; run += x; }
                }
            }
            SYNC();
            PAR(tid) {
                uint64_t at = cnt[tile] + scan[tid] + grp[KMER_GROUP + tid / KMER_GROUP];
                const uint64_t r0 = t0 + (uint64_t)tid * KMER_LANE;
                ck_each_run(rk + tid * CK_LANE_PITCH, r0, n, TL(st, tid, 0), TL(st, tid, 1), TL(st, tid, 2),
                            [&](uint64_t hd, uint64_t c, uint64_t occ, uint64_t docs) {
                    if (!ck_passes(q, docs)) return;
                    if (at < cap) {
                        rec[4 * at] = hd;
                        rec[4 * at + 1] = c;
                        rec[4 * at + 2] = occ;
                        rec[4 * at + 3] = docs;
                    }
                    ++at;
                });
            }
            SYNC();
        }
        if (MODE == CK_SHARING) {
            const bool last = tile + K_GRID_DIM >= n_tiles;
            if (++tiles_in == CK_FLUSH_TILES || last) {     // block-uniform
                PAR(tid) {
                    if (TL(reg, tid, 0)) FETCH_ADD_U32(&h[CK_FREQ + 1], TL(reg, tid, 0));
                    if (TL(reg, tid, 1)) FETCH_ADD_U32(&h[CK_FULL], TL(reg, tid, 1));
                    TL(reg, tid, 0) = 0;
                    TL(reg, tid, 1) = 0;
                }
                SYNC();
                PAR(tid) {
                    for (uint32_t b = tid; b < CK_COLS; b += FM_NT) {
                        uint64_t* out = &hist[(uint64_t)K_BLOCK_IDX * CK_COLS + b];
                        *out = (flushed ? *out : 0) + h[b];
                        h[b] = 0;
                    }
                }
                SYNC();
                tiles_in = 0;
                flushed = true;
            }
        }
    }
    if (MODE == CK_SHARING && !flushed) {                   // a workgroup without a tile: its columns are zeros
        PAR(tid) { for (uint32_t b = tid; b < CK_COLS; b += FM_NT) hist[(uint64_t)K_BLOCK_IDX * CK_COLS + b] = 0; }
    }
}

// tot[column] = the sum over the workgroups' rows of hist[workgroup * CK_COLS + column]; a thread per column, coalesced
GLOBAL_FN LAUNCH_BOUNDS(FM_NT) ck_sum_kernel(KCTX const uint64_t* __restrict__ hist, uint32_t rows, uint64_t* __restrict__ tot)
{
    PAR(tid) {
        for (uint32_t b = K_BLOCK_IDX * FM_NT + tid; b < CK_COLS; b += K_GRID_DIM * FM_NT) {
            uint64_t s = 0;
            for (uint32_t g = 0; g < rows; ++g) s += hist[(uint64_t)g * CK_COLS + b];
            tot[b] = s;
        }
    }
}

}  // namespace caps
