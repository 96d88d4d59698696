// caps-sa_amd/csrc/capi_impl.h
//
// Bodies of the C ABI declared in include/caps_sa_hip.h.  Included exactly once by
// caps_sa_hip.hip (product: symbols caps_sa_hip_*) and, for the host emulation used by
// CPU-side logic tests, by tests/emul/emul_lib.cpp (symbols caps_sa_emul_*).
#pragma once
#include <chrono>
#include <cstring>
#include <exception>
#include <functional>
#include <limits>
#include <memory>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "pipeline.h"
#include "shard.h"

#ifndef CAPS_API
#error "define CAPS_API(name) before including capi_impl.h"
#endif

namespace caps {

inline std::string& last_error_ref()
{
    static thread_local std::string s;
    return s;
}

// Runs f(); maps exceptions to the ABI's error codes.
template <typename F> int guarded(F&& f)
{
    try {
        last_error_ref().clear();
        return f();
    } catch (const OomError& e) {
        last_error_ref() = e.what();
        return CAPS_SA_ENOMEM;
    } catch (const HipError& e) {
        last_error_ref() = e.what();
        return CAPS_SA_EHIP;
    } catch (const AlphabetError& e) {
        last_error_ref() = e.what();
        return CAPS_SA_EALPHABET;
    } catch (const std::bad_alloc&) {
        last_error_ref() = "host allocation failed";
        return CAPS_SA_ENOMEM;
    } catch (const std::exception& e) {
        last_error_ref() = e.what();
        return CAPS_SA_EINVAL;
    }
}

inline int fail(int code, const char* msg)
{
    last_error_ref() = msg;
    return code;
}

// RAII device allocations of one call.
struct DevAllocs {
    Backend& be;
    std::vector<void*> ptrs;
    explicit DevAllocs(Backend& b) : be(b) {}
    ~DevAllocs() { for (void* p : ptrs) be.free(p); }
    template <typename T> T* get(size_t count)
    {
        T* p = static_cast<T*>(be.alloc(count * sizeof(T)));
        ptrs.push_back(p);
        return p;
    }
};

// ---- what every entry point with a workspace shares -----------------------------------------------------------------------------------
// A plan's `bytes` is its layout alone, every part at a multiple of WS_ALIGN (pipeline.h align_up).  What a *_workspace_bytes query
// reports is ws_reported(bytes): WS_ALIGN more, the most that aligning a caller's pointer up can cost.  ws_check refuses a caller's
// workspace that cannot hold the layout, ws_carve gives the aligned base -- in the caller's workspace, or in an allocation of the
// call's own when there is none.
inline uint64_t ws_reported(size_t layout_bytes) { return layout_bytes + WS_ALIGN; }
// WS_SLACK: the bytes that aligning this pointer loses are subtracted first; WS_STRICT: anything below the reported size is refused
enum WsRule { WS_SLACK, WS_STRICT };
inline int ws_check(void* workspace, uint64_t workspace_bytes, size_t layout_bytes, const char* too_small, WsRule rule = WS_SLACK)
{
    if (!workspace) return CAPS_SA_OK;
    char* ws = static_cast<char*>(workspace);
    const uint64_t lost = rule == WS_STRICT ? WS_ALIGN : (uint64_t)(align_up(ws) - ws);
    if (workspace_bytes < layout_bytes + lost) return fail(CAPS_SA_EINVAL, too_small);
    return CAPS_SA_OK;
}
inline char* ws_carve(DevAllocs& da, void* workspace, size_t layout_bytes)
{
    return align_up(workspace ? static_cast<char*>(workspace) : da.get<char>(ws_reported(layout_bytes)));
}

// the arguments of a size query over (n, idx_bytes); n_limit: the queries that also refuse n above 2^60
inline int check_size_query(uint64_t n, int idx_bytes, const uint64_t* bytes, bool n_limit = true)
{
    if (!bytes || (idx_bytes != 4 && idx_bytes != 8)) return fail(CAPS_SA_EINVAL, "bad argument");
    if (idx_bytes == 4 && n > 0xFFFFFFFFull) return fail(CAPS_SA_EINVAL, "n does not fit 32-bit indices (use idx_bytes = 8)");
    if (n_limit && n > (1ull << 60)) return fail(CAPS_SA_EINVAL, "n is too large");
    return CAPS_SA_OK;
}
// n against the index type, and the arrays of n entries (any_null: one of them is missing)
template <typename idx_t> int check_arrays(uint64_t n, bool any_null, const char* null_msg)
{
    if (n > (uint64_t)std::numeric_limits<idx_t>::max()) return fail(CAPS_SA_EINVAL, "n does not fit 32-bit indices (use the _u64 entry point)");
    if (n > (1ull << 60)) return fail(CAPS_SA_EINVAL, "n is too large");
    if (n && any_null) return fail(CAPS_SA_EINVAL, null_msg);
    return CAPS_SA_OK;
}

// host SA and LCP of a host form, uploaded into buffers of the call's own
template <typename idx_t> struct UploadedSaLcp {
    idx_t* sa = nullptr;
    idx_t* lcp = nullptr;
    UploadedSaLcp(Backend& be, DevAllocs& da, const idx_t* SA, const idx_t* LCP, uint64_t n)
    {
        if (!n) return;
        sa = da.get<idx_t>(n);
        lcp = da.get<idx_t>(n);
        be.h2d(sa, SA, n * sizeof(idx_t));
        be.h2d(lcp, LCP, n * sizeof(idx_t));
    }
};

template <typename idx_t> int check_common(const void* T, uint64_t n, uint64_t max_context)
{
    if (n && !T) return fail(CAPS_SA_EINVAL, "null text");
    if (n > (uint64_t)std::numeric_limits<idx_t>::max())
        return fail(CAPS_SA_EINVAL, "n does not fit the index type (use the _u64 entry point, src/main.cpp:76)");
    // bounded context (csrc/bounded.h): defined where the reference is -- n >= 32 and at least two subproblems
    if (max_context != 0 && max_context < n && n < 32)
        return fail(CAPS_SA_EUNSUPPORTED, "bounded max_context needs n >= 32 (the reference is undefined below that)");
    return CAPS_SA_OK;
}

int set_device(int device);   // defined by the including translation unit

// waves / sink: Builder::set_waves (the host-buffer entry point streams finished slices of the result out while the rest is sorted)
inline uint64_t wave_scratch_elems(uint64_t n, uint32_t waves) { return std::max<uint64_t>(4 * TILE_E, (n / waves) * 3 / 2 + 2 * TILE_E); }
template <typename idx_t> inline size_t wave_scratch_bytes(uint64_t elems)
{
    return align_up(elems * sizeof(uint64_t)) + 2 * align_up(elems * sizeof(idx_t)) + WS_ALIGN;
}
template <typename idx_t>
int build_device(const void* dT, uint64_t n, uint64_t p_arg, uint64_t max_context, void* dSA, void* dLCP, void* workspace,
                 uint64_t workspace_bytes, void* stream, caps_sa_stats* stats, uint32_t waves = 1, WaveSink* sink = nullptr,
                 bool* sink_served = nullptr, int arena_bits = 0)
{
    // arena_bits: the code width the workspace's text arena was sized for (0: told by the size of the workspace)
    if (int rc = check_common<idx_t>(dT, n, max_context)) return rc;
    if (n && (!dSA || !dLCP)) return fail(CAPS_SA_EINVAL, "null output");
    return guarded([&]() -> int {
        Backend be(static_cast<decltype(Backend::stream)>(stream));
        DevAllocs da(be);
        Plan<idx_t> need = make_plan<idx_t>(n, p_arg, nullptr);
        char* base = static_cast<char*>(workspace);
        int text_bits = arena_bits == 2 ? 2 : 8;
        if (!base) base = da.get<char>(need.bytes);
        else if (arena_bits == 2) {
            if (workspace_bytes < make_plan<idx_t>(n, p_arg, nullptr, 2).bytes) return fail(CAPS_SA_EINVAL, "workspace too small");
        } else if (workspace_bytes < need.bytes) {
            // a workspace of caps_sa_hip_workspace_bytes_ex(.., 2, ..): the text arena holds 2-bit codes only
            if (workspace_bytes < make_plan<idx_t>(n, p_arg, nullptr, 2).bytes) return fail(CAPS_SA_EINVAL, "workspace too small");
            text_bits = 2;
        }
        // carve from a 256-byte aligned base
        char* aligned = align_up(base);
        Plan<idx_t> pl = make_plan<idx_t>(n, p_arg, aligned, text_bits);
        Builder<idx_t> b(be, pl);
        ElemBuf<idx_t> scratch;
        uint64_t scratch_elems = 0;
        if (waves > 1 && sink) {                         // the waves' work arrays, behind the plan in the caller's workspace
            scratch_elems = wave_scratch_elems(n, waves);
            char* sb = aligned + align_up(pl.bytes);
            if (workspace && static_cast<char*>(workspace) + workspace_bytes >= sb + wave_scratch_bytes<idx_t>(scratch_elems)) {
                scratch.key = reinterpret_cast<uint64_t*>(sb);
                scratch.sa = reinterpret_cast<idx_t*>(sb + align_up(scratch_elems * sizeof(uint64_t)));
                scratch.lcp = reinterpret_cast<idx_t*>(reinterpret_cast<char*>(scratch.sa) + align_up(scratch_elems * sizeof(idx_t)));
                scratch.region_bytes = wave_scratch_bytes<idx_t>(scratch_elems);
            } else scratch_elems = 0;
        }
        b.set_waves(waves, sink, scratch, scratch_elems);
        if (sink) sink->text(pl.P, pl.lut);
        if (max_context != 0 && max_context < n && pl.p < 2)
            return fail(CAPS_SA_EUNSUPPORTED, "bounded max_context needs at least two subproblems (the reference divides by zero there)");
        b.build(static_cast<const uint8_t*>(dT), static_cast<idx_t*>(dSA), static_cast<idx_t*>(dLCP), stats, max_context);
        if (sink_served) *sink_served = b.sink_served();
        return CAPS_SA_OK;
    });
}

// Results of the host-buffer entry point leave the device slice by slice: when a wave of groups has been sorted (its slice of
// SA / LCP is final), a second stream waits for that point of the build's stream and copies the slice to the caller's arrays
// while the next wave is sorted -- the D2H of 2 n indices (24 GB at C3: 420 ms at the link rate) then hides the rest of the
// build instead of following it.  (The upload of T cannot hide anything: sampling and level A need the whole text.)
//
// LCP as bytes (32-bit indices; lcp_narrow_kernel): on the link the LCP array is a quarter of its size -- 15 GB instead of 24 at C3.
// Per slice, on the copy stream: narrow on the device, copy the bytes into a page-locked staging array, copy the SA slice; a host
// thread waits for the bytes and widens them into the caller's array (a few worker threads, streaming stores) while the SA slice
// and the next slices are on the link.  Values of 255 and more travel as (position, value) pairs at the end; when there are more of
// them than the list holds (a^n: every value), the whole array is copied at full width as before.
inline uint32_t host_worker_threads()
{
    if (const char* e = std::getenv("CAPS_SA_HOST_THREADS")) return (uint32_t)std::max(1, std::atoi(e));
    uint32_t hw = std::thread::hardware_concurrency();
    // (a container's CPU quota is usually far below the node's thread count: the GPU boxes show 256 and grant 16)
    FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r");
    if (f) {
        long long q = 0, per = 0;
        char qs[32] = {0};
        if (std::fscanf(f, "%31s %lld", qs, &per) == 2 && std::strcmp(qs, "max") != 0 && per > 0) {
            q = std::atoll(qs);
            if (q > 0) hw = std::min<uint32_t>(hw ? hw : 1u, (uint32_t)std::max<long long>(1, (q + per - 1) / per));
        }
        std::fclose(f);
    }
    return std::max(1u, std::min(hw ? hw : 1u, 32u));
}

// out[i] = in[i] for i in [0, cnt): bytes to 32-bit values, with streaming stores where the compiler has them (the 12 GB written at
// C3 would otherwise be read first, line by line)
inline void widen_bytes(const uint8_t* in, uint32_t* out, uint64_t cnt)
{
    uint64_t i = 0;
#if defined(__clang__) && defined(__SSE2__)
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    for (; i < cnt && (reinterpret_cast<uintptr_t>(out + i) & 15u); ++i) out[i] = in[i];
    for (; i + 4 <= cnt; i += 4) {
        const v4u v = {in[i], in[i + 1], in[i + 2], in[i + 3]};
        __builtin_nontemporal_store(v, reinterpret_cast<v4u*>(out + i));
    }
#endif
    for (; i < cnt; ++i) out[i] = in[i];
}

// BWT of the suffix-array slice dSA[0 .. cnt) (ranks first .. first + cnt) into out[0 .. cnt), on be's stream (kernels.h bwt_kernel).
// *dprimary is written only when the slice holds the entry 0: the caller arms it with UINT64_MAX.
template <typename idx_t>
void launch_bwt(Backend& be, const uint8_t* dT, uint64_t n, const idx_t* dSA, uint64_t first, uint64_t cnt, uint8_t* out, uint64_t* dprimary)
{
    if (!cnt) return;
    const uint64_t rounds = (cnt + 256ull * BWT_PER - 1) / (256ull * BWT_PER);
    CAPS_LAUNCH((bwt_kernel<idx_t>), capped_grid(std::min<uint64_t>(rounds, 8192), 256), 256, be, dT, n, dSA, first, cnt, out, dprimary);
}

template <typename idx_t> struct HostCopySink : WaveSink {
    decltype(Backend::stream) copy_stream;
    idx_t *SA, *LCP;
    const idx_t *dSA, *dLCP;
    uint64_t copied = 0;
    // LCP as bytes (null: plain copies)
    uint8_t* d8 = nullptr;             // device: the bytes
    uint64_t* dexc = nullptr;          // device: exceptions, (position << 32 | value)
    uint64_t* dexc_count = nullptr;
    uint64_t exc_cap = 0;
    // host, page-locked: the bytes land in CHUNKS of chunk_bytes (chunk c = positions [c * chunk_bytes, ...)), allocated one after
    // the other by a thread of their own while the text is uploaded and the first slices are sorted: page-locking memory costs ~4 ms
    // per 64 MB -- 240 ms for a C3-sized array, which a first call would otherwise pay up front -- and a slice only needs the chunks
    // under it (chunk_ready blocks until chunk c exists).  Kept between calls with the device block.
    std::vector<char*>* chunks = nullptr;
    uint64_t chunk_bytes = 0;
    std::function<void(uint64_t)> chunk_ready;
    std::vector<uint64_t> hexc_store;  // host: the exceptions (pageable: a few MB at the end)
    uint64_t* hexc = nullptr;
    uint32_t workers = 1;
    struct Task { BackendEvent ev; uint64_t base, cnt; };
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Task> tasks;
    bool closing = false, busy = false;
    std::thread dispatcher;
    std::exception_ptr failure;
    // the BWT (null: not asked for): every slice gathered from the build's packed text on the copy stream (bwt_packed_kernel), then
    // copied to BWT + base; the paths that stream nothing gather once from the raw text dT after the build.  Its own device bytes
    // (dBWT, dprimary), apart from the LCP bytes above.
    uint64_t n = 0;
    uint8_t* dBWT = nullptr;
    uint64_t* dprimary = nullptr;
    uint8_t* BWT = nullptr;
    // the packed text and its byte -> code table (WaveSink::text); pbits = 0 until the first slice has made code2byte from the table
    const uint32_t* Ptext = nullptr;
    const uint8_t* dlut = nullptr;
    int pbits = 0;
    uint32_t code2byte = 0;
    void text(const uint32_t* P, const uint8_t* lut) override { Ptext = P; dlut = lut; }

    bool narrow() const { return d8 != nullptr; }
    // f(chunk pointer + offset, position, length) for the pieces of [base, base + cnt) chunk by chunk
    template <typename F> void for_pieces(uint64_t base, uint64_t cnt, F&& f)
    {
        for (uint64_t pos = base; pos < base + cnt;) {
            const uint64_t c = pos / chunk_bytes, off = pos - c * chunk_bytes;
            const uint64_t len = std::min<uint64_t>(chunk_bytes - off, base + cnt - pos);
            f(c, off, pos, len);
            pos += len;
        }
    }
    void widen_slice(uint64_t base, uint64_t cnt)
    {
        if (sizeof(idx_t) != 4) return;
        for_pieces(base, cnt, [this](uint64_t c, uint64_t off, uint64_t pos, uint64_t len) {
            uint32_t* out = reinterpret_cast<uint32_t*>(LCP) + pos;
            const uint8_t* in = reinterpret_cast<const uint8_t*>((*chunks)[c]) + off;
#ifdef CAPS_EMUL
            widen_bytes(in, out, len);
#else
            const uint32_t K = (uint32_t)std::min<uint64_t>(workers, std::max<uint64_t>(1, len >> 20));
            if (K <= 1) { widen_bytes(in, out, len); return; }
            std::vector<std::thread> th;
            const uint64_t per = ((len + K - 1) / K + 63) & ~uint64_t(63);
            for (uint32_t k = 0; k < K; ++k) {
                const uint64_t a = std::min<uint64_t>(len, (uint64_t)k * per), b = std::min<uint64_t>(len, a + per);
                if (a < b) th.emplace_back([=] { widen_bytes(in + a, out + a, b - a); });
            }
            for (auto& t : th) t.join();
#endif
        });
    }
    void start()
    {
#ifndef CAPS_EMUL
        if (!narrow()) return;
        dispatcher = std::thread([this] {
            for (;;) {
                Task t;
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [this] { return closing || !tasks.empty(); });
                    if (tasks.empty()) return;
                    t = tasks.front();
                    tasks.pop_front();
                    busy = true;
                }
                try {
                    Backend::wait_event(t.ev);
                    Backend::destroy_event(t.ev);
                    widen_slice(t.base, t.cnt);
                } catch (...) { std::lock_guard<std::mutex> lk(mu); failure = std::current_exception(); }
                { std::lock_guard<std::mutex> lk(mu); busy = false; }
                cv.notify_all();
            }
        });
#endif
    }
    void drain()                       // every slice handed over so far has been widened
    {
#ifndef CAPS_EMUL
        if (!dispatcher.joinable()) return;
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [this] { return tasks.empty() && !busy; });
#endif
    }
    void stop()
    {
#ifndef CAPS_EMUL
        if (!dispatcher.joinable()) return;
        { std::lock_guard<std::mutex> lk(mu); closing = true; }
        cv.notify_all();
        dispatcher.join();
#endif
    }
    ~HostCopySink() override { stop(); }

    void wave_done(Backend& be, uint64_t base, uint64_t cnt) override
    {
        Backend::stream_wait(copy_stream, be.record());
        if (dBWT) {
            Backend cb(copy_stream);
            if (!pbits) {                                   // code -> byte from the build's table (written by prepare_text, long before the first slice):
                                                            // 2-bit tables hold codes 0..3 and 0xFF (absent bytes), 8-bit ones 256 distinct codes
                uint8_t lut[256];
                Backend::d2h_on(copy_stream, lut, dlut, 256);
                Backend::sync_stream(copy_stream);
                int distinct = 0;
                bool seen[256] = {false};
                for (int c = 0; c < 256; ++c) if (!seen[lut[c]]) { seen[lut[c]] = true; ++distinct; }
                pbits = distinct > 5 ? 8 : 2;
                code2byte = 0;
                if (pbits == 2) for (int c = 0; c < 256; ++c) if (lut[c] < 4) code2byte |= (uint32_t)c << (8 * lut[c]);
            }
            const uint64_t rounds = (cnt + 256ull * BWT_PER - 1) / (256ull * BWT_PER);
            const uint32_t g = capped_grid(std::min<uint64_t>(rounds, 8192), 256);
            if (cnt && pbits == 2)
                CAPS_LAUNCH((bwt_packed_kernel<idx_t, 2>), g, 256, cb, Ptext, n, dSA + base, base, cnt, dBWT + base, dprimary, code2byte);
            else if (cnt)
                CAPS_LAUNCH((bwt_packed_kernel<idx_t, 8>), g, 256, cb, Ptext, n, dSA + base, base, cnt, dBWT + base, dprimary, code2byte);
        }
        if (narrow()) {
            Backend cb(copy_stream);
            const uint64_t rounds = (cnt + 256ull * NARROW_PER - 1) / (256ull * NARROW_PER);
            CAPS_LAUNCH(lcp_narrow_kernel, capped_grid(std::min<uint64_t>(rounds, 4096), 256), 256, cb,
                        reinterpret_cast<const uint32_t*>(dLCP) + base, cnt, base, d8 + base, dexc_count, exc_cap, dexc);
            for_pieces(base, cnt, [this](uint64_t c, uint64_t off, uint64_t pos, uint64_t len) {
                chunk_ready(c);
                Backend::d2h_on(copy_stream, (*chunks)[c] + off, d8 + pos, len);
            });
            const BackendEvent ev = Backend::record_on(copy_stream);
            Backend::d2h_on(copy_stream, SA + base, dSA + base, cnt * sizeof(idx_t));
#ifdef CAPS_EMUL
            widen_slice(base, cnt);
            (void)ev;
#else
            { std::lock_guard<std::mutex> lk(mu); tasks.push_back(Task{ev, base, cnt}); }
            cv.notify_all();
#endif
        } else {
            Backend::d2h_on(copy_stream, SA + base, dSA + base, cnt * sizeof(idx_t));
            Backend::d2h_on(copy_stream, LCP + base, dLCP + base, cnt * sizeof(idx_t));
        }
        if (dBWT) Backend::d2h_on(copy_stream, BWT + base, dBWT + base, cnt);
        copied += cnt;
    }
    void reset(Backend&) override
    {
        Backend::sync_stream(copy_stream);                  // nothing reads the device arrays any more
        drain();
        if (narrow()) { Backend::memset_on(copy_stream, dexc_count, 0, sizeof(uint64_t)); Backend::sync_stream(copy_stream); }
        if (dprimary) { Backend::memset_on(copy_stream, dprimary, 0xFF, sizeof(uint64_t)); Backend::sync_stream(copy_stream); }   // the slices come again
        copied = 0;
    }
    // after the last slice: the values of 255 and more.  false: more of them than the list holds -- the caller copies LCP at full width
    bool finish_lcp(uint64_t n)
    {
        if (!narrow()) { Backend::sync_stream(copy_stream); return true; }        // (the last copies have landed)
        uint64_t ne = 0;
        Backend::d2h_on(copy_stream, &ne, dexc_count, sizeof(uint64_t));
        Backend::sync_stream(copy_stream);
        drain();
        if (failure) std::rethrow_exception(failure);
        if (ne > exc_cap) return false;
        if (ne) {
            hexc_store.resize(ne);
            hexc = hexc_store.data();
            Backend::d2h_on(copy_stream, hexc, dexc, ne * sizeof(uint64_t));
            Backend::sync_stream(copy_stream);
            auto patch = [this, n](uint64_t a, uint64_t b) {
                for (uint64_t i = a; i < b; ++i) {
                    const uint64_t pos = hexc[i] >> 32;
                    if (pos < n) LCP[pos] = (idx_t)(hexc[i] & 0xFFFFFFFFull);
                }
            };
#ifdef CAPS_EMUL
            patch(0, ne);
#else
            const uint32_t K = (uint32_t)std::min<uint64_t>(workers, std::max<uint64_t>(1, ne >> 16));
            if (K <= 1) patch(0, ne);
            else {                                           // (scattered stores: a few million of them on a repeat-rich genome)
                std::vector<std::thread> th;
                for (uint32_t k = 0; k < K; ++k) th.emplace_back(patch, ne * k / K, ne * (k + 1) / K);
                for (auto& t : th) t.join();
            }
#endif
        }
        return true;
    }
};
#ifndef CAPS_HOST_WAVES
#define CAPS_HOST_WAVES 12
#endif

// Device memory of the host-buffer entry points, kept between calls: hipMalloc + hipFree of the
// text, the result arrays and the workspace cost far more than the build they serve (n = 1e9:
// 1.2 s against 28 ms).  One grow-only block per process, re-allocated when a larger build or
// another device asks; released by caps_sa_hip_release_cache() (or at process exit).  Calls of the
// host-buffer entry points are serialised on it.
struct HostPathCache {
    std::mutex mu;
    int device = -1;
    char* base = nullptr;
    size_t bytes = 0;
    std::vector<char*> host_chunks;    // page-locked staging of the LCP bytes (HostCopySink), host_chunk_bytes each
    size_t host_chunk_bytes = 0;
    uint64_t calls = 0;                // host-buffer builds of this process so far
    // the index blob at the head of the block (the host queries of the FM and LCE indexes): the host blob it was uploaded from, its
    // size, its header and a sum over a stride of its body; null when anything else has used the block since
    const void* blob_host = nullptr;
    uint64_t blob_bytes = 0, blob_sum = 0;
    uint64_t blob_hdr[32] = {};
};
inline HostPathCache& host_cache()
{
    static HostPathCache c;
    return c;
}

inline void release_host_cache_locked(HostPathCache& c)
{
    if (c.base) {
        Backend be(nullptr);
        be.free(c.base);
    }
    for (char* q : c.host_chunks) Backend::host_free(q);
    c.host_chunks.clear();
    c.host_chunk_bytes = 0;
    c.base = nullptr;
    c.bytes = 0;
    c.device = -1;
    c.blob_host = nullptr;
}

// The host-path block with room for `total` bytes on `device`: kept when it is large enough, else released and allocated again
// (the page-locked staging chunks of the builds survive that).  -> whether it was allocated by this call.
inline bool host_block(HostPathCache& hc, Backend& be, int device, size_t total)
{
    if (hc.device == device && hc.bytes >= total) return false;
    std::vector<char*> keep;
    keep.swap(hc.host_chunks);
    const size_t keep_bytes = hc.host_chunk_bytes;
    release_host_cache_locked(hc);
    hc.host_chunks.swap(keep);
    hc.host_chunk_bytes = keep_bytes;
    hc.base = static_cast<char*>(be.alloc(total));
    hc.bytes = total;
    hc.device = device;
    return true;
}

// BWT (build_bwt): null, or n bytes of the caller's that receive the BWT slice by slice with the rest of the result (HostCopySink);
// *primary then the rank of the suffix 0.
template <typename idx_t>
int build_host(const char* T, uint64_t n, uint64_t p_arg, uint64_t max_context, idx_t* SA, idx_t* LCP, int device,
               caps_sa_stats* stats, uint8_t* BWT = nullptr, uint64_t* primary = nullptr)
{
    if (int rc = check_common<idx_t>(T, n, max_context)) return rc;
    if (n && (!SA || !LCP)) return fail(CAPS_SA_EINVAL, "null output");
    const bool want_bwt = BWT != nullptr && n != 0;
    DeviceScope restore_device_;
    if (int rc = set_device(device)) return rc;
    return guarded([&]() -> int {
        HostPathCache& hc = host_cache();
        std::lock_guard<std::mutex> lock(hc.mu);
        Backend be(nullptr);
        hc.blob_host = nullptr;                                // (the block is this build's now)
        // the text arena is sized for 2-bit codes when the first MiB of the text shows at most 4 distinct bytes (a text that
        // turns out to have more is built again below with the arena of 8-bit codes)
        int text_bits = 8;
        {
            bool seen[256] = {false};
            int sigma = 0;
            const uint64_t look = n < (1u << 20) ? n : (1u << 20);
            for (uint64_t i = 0; i < look && sigma <= 4; ++i)
                if (!seen[(uint8_t)T[i]]) { seen[(uint8_t)T[i]] = true; ++sigma; }
            if (sigma <= 4 && !std::getenv("CAPS_SA_FULL_ALPHABET")) text_bits = 2;
        }
        const uint64_t earlier_calls = hc.calls++;
        for (;; text_bits = 8) {
        const Plan<idx_t> need = make_plan<idx_t>(n, p_arg, nullptr, text_bits);
        const size_t off_sa = align_up(n ? n : 1), off_lcp = off_sa + align_up((n ? n : 1) * sizeof(idx_t));
        const size_t off_ws = off_lcp + align_up((n ? n : 1) * sizeof(idx_t));
        // waves pay when the build is long enough to hide: measured at C2 (256 Mi: 5 ms of build against 38 ms of copies) twelve
        // waves cost 14 ms (per-wave host synchronisations, 24 copies instead of 2), at C3 (3e9) they save 31 of 524 ms
        uint32_t waves = n >= (400ull << 20) ? CAPS_HOST_WAVES : 1u;
        if (const char* e = std::getenv("CAPS_SA_HOST_WAVES")) waves = (uint32_t)std::max(1, std::atoi(e));
        // LCP as bytes: with waves (the builds long enough for the link to matter), 32-bit indices -- and from the SECOND host build of
        // a process on: the page-locked staging costs ~240 ms to allocate at C3 (measured: not hidden by allocating it on a thread
        // beside the upload -- the runtime serialises the two), which a process that builds once (the CLI) would pay for a saving
        // of 150 ms; one that builds again and again pays it once.  CAPS_SA_HOST_NARROW_LCP=0 / 1: never / from the first build.
        bool narrow = sizeof(idx_t) == 4 && waves > 1 && earlier_calls > 0;
        if (const char* e = std::getenv("CAPS_SA_HOST_NARROW_LCP")) narrow = sizeof(idx_t) == 4 && std::atoi(e) != 0;
        // (the device block has room for the bytes from the first build on: growing it by a second build would free and re-allocate
        // ~130 GB, which takes seconds)
        const bool narrow_later = sizeof(idx_t) == 4 && waves > 1 && !(std::getenv("CAPS_SA_HOST_NARROW_LCP") && !narrow);
        const uint64_t exc_cap = narrow || narrow_later ? std::max<uint64_t>(1024, n / 32) : 0;
        const size_t narrow_dev = narrow || narrow_later ? align_up(n) + align_up((exc_cap + 1) * sizeof(uint64_t)) + 512 : 0;
        const size_t ws_room = need.bytes + 1024 + wave_scratch_bytes<idx_t>(wave_scratch_elems(n, waves));
        // the BWT's bytes and its primary index, behind everything else (builds without a BWT ask for the block they always did)
        const size_t off_bwt = off_ws + align_up(ws_room) + align_up(narrow_dev);
        const size_t total = want_bwt ? off_bwt + align_up(n) + 512 : off_ws + ws_room + narrow_dev;
        const auto a0 = std::chrono::steady_clock::now();
        if (host_block(hc, be, device, total) && std::getenv("CAPS_SA_DEBUG_ALLOC"))
            std::fprintf(stderr, "[alloc] device block of %zu bytes: %.1f ms\n", total,
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a0).count());
        // the page-locked chunks for the LCP bytes, allocated beside the upload (HostCopySink::chunks)
        constexpr uint32_t N_CHUNKS = 16;
        const uint64_t chunk_bytes = narrow ? align_up((n + N_CHUNKS - 1) / N_CHUNKS) : 0;
        const size_t chunks_need = narrow ? (size_t)((n + chunk_bytes - 1) / chunk_bytes) : 0;
        std::thread ring_alloc;
        std::exception_ptr ring_error;
        std::mutex chunk_mu;
        std::condition_variable chunk_cv;
        size_t chunks_done = hc.host_chunks.size();
        if (narrow && (hc.host_chunk_bytes != chunk_bytes || hc.host_chunks.size() < chunks_need)) {
            for (char* q : hc.host_chunks) Backend::host_free(q);
            hc.host_chunks.assign(chunks_need, nullptr);
            hc.host_chunk_bytes = chunk_bytes;
            chunks_done = 0;
            auto alloc = [&, chunks_need, chunk_bytes, device]() {
                try {
                    const auto a0 = std::chrono::steady_clock::now();
                    if (set_device(device) != CAPS_SA_OK) throw HipError("hipSetDevice failed");
                    for (size_t c = 0; c < chunks_need; ++c) {
                        char* q = static_cast<char*>(Backend::host_alloc(chunk_bytes));
                        { std::lock_guard<std::mutex> lk(chunk_mu); hc.host_chunks[c] = q; chunks_done = c + 1; }
                        chunk_cv.notify_all();
                    }
                    if (std::getenv("CAPS_SA_DEBUG_ALLOC"))
                        std::fprintf(stderr, "[alloc] %zu page-locked chunks of %llu bytes: %.1f ms (beside the upload and the first slices)\n", chunks_need,
                                     (unsigned long long)chunk_bytes, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a0).count());
                } catch (...) {
                    { std::lock_guard<std::mutex> lk(chunk_mu); ring_error = std::current_exception(); }
                    chunk_cv.notify_all();
                }
            };
#ifdef CAPS_EMUL
            alloc();
#else
            ring_alloc = std::thread(alloc);
#endif
        }
        struct JoinGuard { std::thread& t; ~JoinGuard() { if (t.joinable()) t.join(); } } ring_join{ring_alloc};
        char* base = align_up(hc.base);
        uint8_t* dT = reinterpret_cast<uint8_t*>(base);
        idx_t* dSA = reinterpret_cast<idx_t*>(base + off_sa);
        idx_t* dLCP = reinterpret_cast<idx_t*>(base + off_lcp);
        if (std::getenv("CAPS_SA_DEBUG_ALLOC")) {       // where the build's arrays sit (a faulting address can then be placed)
            const Plan<idx_t> pl = make_plan<idx_t>(n, p_arg, base + off_ws, text_bits);
            std::fprintf(stderr, "[alloc] block %p + %zu | T %p SA %p LCP %p ws %p | P %p A.key %p A.sa %p A.lcp %p B.key %p B.sa %p B.lcp %p seg1.rec %p SA_.key %p "
                         "Pm %p desc %p bk.params %p bk.count %p bk.sub.rec %p end %p\n", (void*)hc.base, hc.bytes, (void*)dT, (void*)dSA, (void*)dLCP,
                         (void*)(base + off_ws), (void*)pl.P, (void*)pl.A.key, (void*)pl.A.sa, (void*)pl.A.lcp, (void*)pl.B.key, (void*)pl.B.sa, (void*)pl.B.lcp,
                         (void*)pl.seg1.tile_rec, (void*)pl.SA_.key, (void*)pl.Pm, (void*)pl.desc, (void*)pl.bk.params, (void*)pl.bk.count,
                         (void*)pl.bk.sub.tile_rec, (void*)(base + off_ws + pl.bytes));
        }
        BackendEvent h0 = be.record();
        be.h2d(dT, T, n);
        BackendEvent h1 = be.record();
        be.sync();
        caps_sa_stats local;
        HostCopySink<idx_t> sink;
        sink.copy_stream = Backend::create_stream();
        sink.SA = SA;
        sink.LCP = LCP;
        sink.dSA = dSA;
        sink.dLCP = dLCP;
        if (narrow) {
            char* nb = base + off_ws + align_up(ws_room);
            sink.d8 = reinterpret_cast<uint8_t*>(nb);
            sink.dexc = reinterpret_cast<uint64_t*>(nb + align_up(n));
            sink.dexc_count = sink.dexc + exc_cap;
            sink.exc_cap = exc_cap;
            sink.chunks = &hc.host_chunks;
            sink.chunk_bytes = chunk_bytes;
            sink.chunk_ready = [&](uint64_t c) {
                std::unique_lock<std::mutex> lk(chunk_mu);
                chunk_cv.wait(lk, [&] { return chunks_done > c || ring_error; });
                if (ring_error) std::rethrow_exception(ring_error);
            };
            sink.workers = host_worker_threads();
            be.memset(sink.dexc_count, 0, sizeof(uint64_t));
            be.sync();
        }
        if (want_bwt) {
            sink.n = n;
            sink.dBWT = reinterpret_cast<uint8_t*>(base + off_bwt);
            sink.dprimary = reinterpret_cast<uint64_t*>(base + off_bwt + align_up(n));
            sink.BWT = BWT;
            be.memset(sink.dprimary, 0xFF, sizeof(uint64_t));
            be.sync();
        }
        sink.start();
        struct StreamGuard { decltype(Backend::stream) s; ~StreamGuard() { Backend::destroy_stream(s); } } guard{sink.copy_stream};
        bool served = false;
        const auto t0 = std::chrono::steady_clock::now();
        int rc = build_device<idx_t>(dT, n, p_arg, max_context, dSA, dLCP, base + off_ws, ws_room - 256, nullptr, &local, waves,
                                     &sink, &served, text_bits);
        if (rc == CAPS_SA_EALPHABET && text_bits == 2) { Backend::sync_stream(sink.copy_stream); sink.drain(); sink.stop(); continue; }
        if (rc) { Backend::sync_stream(sink.copy_stream); sink.drain(); return rc; }
        bool lcp_as_bytes = sink.narrow();
        if (!served || sink.copied != n) {           // another construction (samplesort path, tiny input): nothing was streamed out
            Backend::sync_stream(sink.copy_stream);
            sink.drain();
            be.d2h(SA, dSA, n * sizeof(idx_t));
            be.d2h(LCP, dLCP, n * sizeof(idx_t));
            if (want_bwt) {                          // ... and no BWT either: one gather over the whole suffix array
                be.memset(sink.dprimary, 0xFF, sizeof(uint64_t));
                launch_bwt<idx_t>(be, dT, n, dSA, 0, n, sink.dBWT, sink.dprimary);
                be.d2h(BWT, sink.dBWT, n);
            }
            be.sync();
            local.result_waves = 1;
            lcp_as_bytes = false;
        } else if (!sink.finish_lcp(n)) {            // more values of 255 and more than the list holds: LCP at full width
            be.d2h(LCP, dLCP, n * sizeof(idx_t));
            be.sync();
            lcp_as_bytes = false;
        }
        sink.stop();
        if (want_bwt) {                              // (the copy stream has finished: finish_lcp / the branch above synchronised)
            Backend::sync_stream(sink.copy_stream);
            be.d2h(primary, sink.dprimary, sizeof(uint64_t));
            be.sync();
        }
        local.lcp_bytes_on_link = lcp_as_bytes ? 1u : (uint32_t)sizeof(idx_t);
        local.ms_h2d = be.elapsed_ms(h0, h1);
        // build + result copies, overlapped: host wall clock from the launch of the build to the last byte on the host, minus the build
        const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        local.ms_d2h = wall > local.ms_total ? wall - local.ms_total : 0.0;
        if (stats) *stats = local;
        return CAPS_SA_OK;
        }
    });
}

// ---- one process, several GPUs (`devices, n_devices` under construct(); 8e) -----------------------------
// The sharded direct path of shard.h with one Shard per device, driven from this process: text replicated; by default every
// device classifies the WHOLE text (level A) and keeps the groups it owns -- nothing crosses a link -- sorts them, and the
// slices of SA / LCP are copied to the caller's arrays by all devices at once.  With CAPS_SA_SHARD_EXCHANGE=1 every device
// classifies every n_devices-th tile and the blocks of (key, sa) go straight from device to device (peer copies over xGMI:
// inside one process nothing else is needed -- the multi-PROCESS driver, caps_sa_dist.py, does that exchange with RCCL).  A device may be listed more than once (several ranks share it: how a one-GPU box tests this).
// Texts the direct path does not take (long repeats) are built on devices[0] alone.
template <typename idx_t> struct MultiRank {
    int dev = 0;
    decltype(Backend::stream) stream = nullptr;
    std::unique_ptr<Backend> be;
    std::unique_ptr<Shard<idx_t>> sh;
    std::vector<void*> owned;
    uint8_t* dT = nullptr;
    uint64_t *send_k = nullptr, *recv_k = nullptr, *report = nullptr;
    idx_t *send_s = nullptr, *recv_s = nullptr, *dSA = nullptr, *dLCP = nullptr;
    caps_sa_shard_info info;
    std::vector<uint64_t> sc, rc;
    int sort_code = 0;
    double ms_upload = 0, ms_build = 0, ms_download = 0;      // host wall clock of this device's stages (caps_sa_stats)
    template <typename T> T* get(size_t count)
    {
        T* q = static_cast<T*>(be->alloc((count ? count : 1) * sizeof(T)));
        owned.push_back(q);
        return q;
    }
    ~MultiRank()
    {
        if (set_device(dev) != CAPS_SA_OK) return;
        sh.reset();
        if (be) for (void* q : owned) be->free(q);
        be.reset();
        Backend::destroy_stream(stream);
    }
};

// fn(rank) on every rank, each on a thread of its own with its device current (emulation: one after the other)
template <typename R, typename F> void for_each_rank(std::vector<std::unique_ptr<R>>& ranks, F&& fn)
{
#ifdef CAPS_EMUL
    for (auto& r : ranks) fn(*r);
#else
    std::vector<std::thread> th;
    std::vector<std::exception_ptr> err(ranks.size());
    for (size_t i = 0; i < ranks.size(); ++i)
        th.emplace_back([&, i]() {
            try {
                if (set_device(ranks[i]->dev) != CAPS_SA_OK) throw HipError("hipSetDevice failed");
                fn(*ranks[i]);
            } catch (...) { err[i] = std::current_exception(); }
        });
    for (auto& t : th) t.join();
    for (auto& e : err) if (e) std::rethrow_exception(e);
#endif
}

template <typename idx_t>
int build_host(const char* T, uint64_t n, uint64_t p_arg, uint64_t max_context, idx_t* SA, idx_t* LCP, int device,
               caps_sa_stats* stats, uint8_t* BWT, uint64_t* primary);

template <typename idx_t>
int build_multi(const char* T, uint64_t n, uint64_t p_arg, uint64_t max_context, idx_t* SA, idx_t* LCP, const int* devices,
                int n_devices, caps_sa_stats* stats)
{
    if (!devices || n_devices < 1) return fail(CAPS_SA_EINVAL, "no devices");
    if (int rc = check_common<idx_t>(T, n, max_context)) return rc;
    if (n && (!SA || !LCP)) return fail(CAPS_SA_EINVAL, "null output");
    if (n_devices == 1) return build_host<idx_t>(T, n, p_arg, max_context, SA, LCP, devices[0], stats);
    // bounded context: the reference's merge trees are one sequence (csrc/bounded.h); built on devices[0] alone
    if (max_context != 0 && max_context < n) return build_host<idx_t>(T, n, p_arg, max_context, SA, LCP, devices[0], stats);
    DeviceScope restore_device_;
    for (int i = 0; i < n_devices; ++i)
        if (int rc = set_device(devices[i])) return rc;
    int fallback = CAPS_SA_FB_NONE;
    const int rc = guarded([&]() -> int {
        using clock = std::chrono::steady_clock;
        const auto t0 = clock::now();
        uint32_t p_eff = 0, ppp = 0;
        effective_params(n, p_arg, &p_eff, &ppp);
        if (p_eff < 2) { fallback = CAPS_SA_FB_SHAPE; return CAPS_SA_OK; }
        const int world = n_devices;
        auto ms = [](clock::time_point a, clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        std::vector<std::unique_ptr<MultiRank<idx_t>>> ranks;
        for (int r = 0; r < world; ++r) {
            std::unique_ptr<MultiRank<idx_t>> q(new MultiRank<idx_t>);
            q->dev = devices[r];
            if (int e = set_device(q->dev)) return e;
            q->stream = Backend::create_stream();
            q->be.reset(new Backend(q->stream));
            q->dT = q->template get<uint8_t>(n);
            ranks.push_back(std::move(q));
        }
        // ---- the text to every device.  ONE upload over PCIe, to ranks[0], in chunks; every chunk goes on from there to the other
        // devices by peer copies (xGMI: one stream per destination, so the seven links of devices[0] work side by side) while the
        // next chunk is still coming up -- H2D + one chunk instead of `world` uploads one after the other from pageable memory
        // (8 x 53 ms at C3-size: more than the sharded build itself).
        {
            MultiRank<idx_t>& root = *ranks[0];
            if (int e = set_device(root.dev)) return e;
            for (int r = 1; r < world; ++r) Backend::enable_peer(root.dev, ranks[r]->dev);
            std::vector<decltype(Backend::stream)> fan((size_t)world, nullptr);
            struct FanGuard { std::vector<decltype(Backend::stream)>& f; ~FanGuard() { for (auto s : f) Backend::destroy_stream(s); } } fan_guard{fan};
            for (int r = 1; r < world; ++r) fan[r] = Backend::create_stream();
#ifdef CAPS_EMUL
            const uint64_t chunk = 1u << 12;                           // small: the CPU tests walk the chunk loop
#else
            const uint64_t chunk = 64ull << 20;
#endif
            for (uint64_t off = 0; off < n; off += chunk) {
                const uint64_t len = n - off < chunk ? n - off : chunk;
                root.be->h2d(root.dT + off, T + off, len);
                const BackendEvent ev = root.be->record();
                for (int r = 1; r < world; ++r) {
                    Backend::stream_wait(fan[r], ev);
                    Backend::peer_copy_on(fan[r], ranks[r]->dT + off, ranks[r]->dev, root.dT + off, root.dev, len);
                }
            }
            root.be->sync();
            root.ms_upload = ms(t0, clock::now());
            for (int r = 1; r < world; ++r) { Backend::sync_stream(fan[r]); ranks[r]->ms_upload = ms(t0, clock::now()); }
            root.be->release_events();
        }
        for (int r = 0; r < world; ++r) {
            MultiRank<idx_t>& q = *ranks[r];
            if (int e = set_device(q.dev)) return e;
            q.sh.reset(new Shard<idx_t>(q.dT, n, p_arg, r, world, q.stream));
            q.sh->info(&q.info);
        }
        if (ranks[0]->info.direct_fallback != CAPS_SA_FB_NONE) { fallback = (int)ranks[0]->info.direct_fallback; return CAPS_SA_OK; }
        const size_t W = (size_t)ranks[0]->info.n_streams + 2;
        for (auto& q : ranks) {
            if (int e = set_device(q->dev)) return e;
            q->send_k = q->template get<uint64_t>(q->info.send_capacity);
            q->send_s = q->template get<idx_t>(q->info.send_capacity);
            if (q->info.exchange) {
                q->recv_k = q->template get<uint64_t>(q->info.capacity);
                q->recv_s = q->template get<idx_t>(q->info.capacity);
            }
            q->dSA = q->template get<idx_t>(q->info.capacity);
            q->dLCP = q->template get<idx_t>(q->info.capacity);
            q->report = q->template get<uint64_t>(W);
        }
        const auto t1 = clock::now();
        auto t2 = t1;
        for (int attempt = 0;; ++attempt) {                       // second attempt: 64-bit keys after a slot overflow under 32
        // ---- level A on every device; the reports; the plan (identical on all ranks)
        for_each_rank(ranks, [&](MultiRank<idx_t>& q) {
            const auto a = clock::now();
            q.sh->scatter(q.send_k, q.send_s, q.report);
            q.be->sync();
            q.ms_build += ms(a, clock::now());
        });
        std::vector<uint64_t> all(W * world);
        for (int r = 0; r < world; ++r) {
            if (int e = set_device(ranks[r]->dev)) return e;
            ranks[r]->be->d2h(all.data() + W * r, ranks[r]->report, W * sizeof(uint64_t));
            ranks[r]->be->sync();
        }
        for (auto& q : ranks) {
            q->sc.assign(world, 0);
            q->rc.assign(world, 0);
            if (int e = set_device(q->dev)) return e;
            const int code = q->sh->plan(all.data(), q->sc.data(), q->rc.data());
            if (code != CAPS_SA_FB_NONE) { fallback = code; return CAPS_SA_OK; }
        }
        // ---- the exchange: block d of rank r's send buffers -> slot r of rank d's receive buffers
        for (auto& q : ranks) q->sh->info(&q->info);              // key_bytes of this attempt
        const bool exchange = ranks[0]->info.exchange != 0;      // (0: every device scattered the whole text and kept its groups)
        for (int r = 0; exchange && r < world; ++r) {
            MultiRank<idx_t>& src = *ranks[r];
            if (int e = set_device(src.dev)) return e;
            uint64_t so = 0;
            for (int d = 0; d < world; ++d) {
                MultiRank<idx_t>& dst = *ranks[d];
                const uint64_t cnt = src.sc[d];
                if (cnt != dst.rc[r]) throw std::runtime_error("send / receive counts disagree");
                uint64_t ro = 0;
                for (int q = 0; q < r; ++q) ro += dst.rc[q];
                const size_t kb = src.info.key_bytes;              // 4 under 32-bit keys: the key arrays are u32 then
                src.be->peer_copy(reinterpret_cast<char*>(dst.recv_k) + ro * kb, dst.dev, reinterpret_cast<const char*>(src.send_k) + so * kb,
                                  src.dev, cnt * kb);
                src.be->peer_copy(dst.recv_s + ro, dst.dev, src.send_s + so, src.dev, cnt * sizeof(idx_t));
                so += cnt;
            }
        }
        for (auto& q : ranks) { if (int e = set_device(q->dev)) return e; q->be->sync(); }
        t2 = clock::now();
        // ---- level B + tile sort of the owned groups; boundary LCPs between the slices
        for_each_rank(ranks, [&](MultiRank<idx_t>& q) {
            const auto a = clock::now();
            q.sort_code = exchange ? q.sh->sort_owned(q.recv_k, q.recv_s, q.dSA, q.dLCP) : q.sh->sort_owned(q.send_k, q.send_s, q.dSA, q.dLCP);
            q.be->sync();
            q.ms_build += ms(a, clock::now());
        });
        int worst = 0;
        for (auto& q : ranks) worst = q->sort_code > worst ? q->sort_code : worst;
        if (worst == CAPS_SA_FB_NONE) break;
        if (attempt > 0) throw std::runtime_error("the sharded direct path failed with 64-bit keys");
        for (auto& q : ranks) q->sh->set_key_bits(64);            // a slot overflowed under 32-bit keys on some rank: all again with 64
        }
        uint64_t prev = ~0ull;
        for (auto& q : ranks) {
            if (int e = set_device(q->dev)) return e;
            q->sh->fix_first_lcp(prev, q->dLCP);
            const uint64_t last = q->sh->last_sa();
            if (last != ~0ull) prev = last;
            q->sh->info(&q->info);
        }
        const auto t3 = clock::now();
        // ---- every device copies its slice to the caller's arrays
        uint64_t covered = 0;
        for (auto& q : ranks) {
            if (q->info.slice_off != covered) throw std::runtime_error("the ranks' slices do not tile the suffix array");
            covered += q->info.recv_total;
        }
        if (covered != n) throw std::runtime_error("the ranks' slices do not cover the suffix array");
        // (every device on a host thread and a stream of its own: the slices leave over all the devices' PCIe links at once)
        for_each_rank(ranks, [&](MultiRank<idx_t>& q) {
            const auto a = clock::now();
            q.be->d2h(SA + q.info.slice_off, q.dSA, q.info.recv_total * sizeof(idx_t));
            q.be->d2h(LCP + q.info.slice_off, q.dLCP, q.info.recv_total * sizeof(idx_t));
            q.be->sync();
            q.ms_download = ms(a, clock::now());
        });
        const auto t4 = clock::now();
        if (stats) {
            *stats = caps_sa_stats();
            stats->n = n;
            stats->idx_bytes = sizeof(idx_t);
            stats->p_eff = ranks[0]->info.p;
            stats->ppp = ranks[0]->info.ppp;
            stats->bits_per_char = ranks[0]->info.bits_per_char;
            stats->path_direct = 1;
            stats->direct_groups = ranks[0]->info.direct_groups;
            stats->direct_quantile = ranks[0]->info.direct_quantile;
            stats->ms_h2d = ms(t0, t1);                       // device setup: allocations + the text to every device
            stats->ms_partition = ms(t1, t2);                 // level A + exchange (host wall clock, all devices)
            stats->ms_merge_partitions = ms(t2, t3);          // level B + tile sort + boundary LCPs
            stats->ms_d2h = ms(t3, t4);
            stats->ms_total = ms(t1, t3);
            for (auto& q : ranks) { stats->slot_splits += q->info.slot_splits; stats->slot_splits_redone += q->info.slot_splits_redone; }
            for (auto& q : ranks) {
                stats->tie_groups_deferred += q->info.tie_groups_deferred;
                stats->tie_levels = std::max(stats->tie_levels, q->info.tie_levels);
            }
            stats->n_devices = (uint32_t)world;
            stats->result_waves = 1;
            stats->ms_upload_min = stats->ms_device_build_min = stats->ms_download_min = 1e300;
            for (auto& q : ranks) {
                stats->ms_upload_max = std::max(stats->ms_upload_max, q->ms_upload);
                stats->ms_upload_min = std::min(stats->ms_upload_min, q->ms_upload);
                stats->ms_device_build_max = std::max(stats->ms_device_build_max, q->ms_build);
                stats->ms_device_build_min = std::min(stats->ms_device_build_min, q->ms_build);
                stats->ms_download_max = std::max(stats->ms_download_max, q->ms_download);
                stats->ms_download_min = std::min(stats->ms_download_min, q->ms_download);
            }
        }
        return CAPS_SA_OK;
    });
    if (rc != CAPS_SA_OK) return rc;
    if (fallback != CAPS_SA_FB_NONE) {
        const int rc1 = build_host<idx_t>(T, n, p_arg, max_context, SA, LCP, devices[0], stats);
        if (rc1 == CAPS_SA_OK && stats && stats->path_fallback == CAPS_SA_FB_NONE) stats->path_fallback = (uint32_t)fallback;
        return rc1;
    }
    return CAPS_SA_OK;
}

template <typename idx_t>
int verify_device(const void* dT, uint64_t n, const void* dSA, const void* dLCP, void* stream, uint64_t* n_errors,
                  uint64_t cnt, uint32_t head)
{
    if (!n_errors) return fail(CAPS_SA_EINVAL, "null n_errors");
    *n_errors = 0;
    if (cnt > n) return fail(CAPS_SA_EINVAL, "more entries than suffixes");
    if (n == 0 || cnt == 0) return CAPS_SA_OK;
    if (!dT || !dSA || !dLCP) return fail(CAPS_SA_EINVAL, "null pointer");
    return guarded([&]() -> int {
        Backend be(static_cast<decltype(Backend::stream)>(stream));
        DevAllocs da(be);
        const size_t words = (n + 31) / 32;
        uint32_t* seen = da.get<uint32_t>(words);
        uint64_t* err = da.get<uint64_t>(1);
        be.memset(seen, 0, words * sizeof(uint32_t));
        be.memset(err, 0, sizeof(uint64_t));
        const uint64_t want = (cnt + 255) / 256;
        CAPS_LAUNCH((verify_kernel<idx_t>), want < 16384 ? want : 16384, 256, be, static_cast<const int8_t*>(dT), n,
                    static_cast<const idx_t*>(dSA), static_cast<const idx_t*>(dLCP), cnt, head, seen, err);
        be.d2h(n_errors, err, sizeof(uint64_t));
        be.sync();
        return CAPS_SA_OK;
    });
}

// construct() plus the BWT (include/caps_sa_hip.h caps_sa_hip_build_bwt_*)
template <typename idx_t>
int build_bwt(const char* T, uint64_t n, uint64_t p_arg, uint64_t max_context, idx_t* SA, idx_t* LCP, uint8_t* BWT, uint64_t* primary,
              int device, caps_sa_stats* stats)
{
    if (!primary) return fail(CAPS_SA_EINVAL, "null primary");
    *primary = ~0ull;
    if (n && !BWT) return fail(CAPS_SA_EINVAL, "null BWT");
    if (max_context != 0 && max_context < n)
        return fail(CAPS_SA_EUNSUPPORTED, "a bounded-context order is not a suffix array: it has no BWT");
    return build_host<idx_t>(T, n, p_arg, max_context, SA, LCP, device, stats, BWT, primary);
}

// The device word bwt_device's kernel writes primary to: one per thread and device, allocated by the first call and kept (a hipFree
// per call would synchronise the whole device every time a slice is transformed).  A call uses it from its memset to its final
// synchronisation, so one per thread suffices.
inline uint64_t* primary_word(Backend& be)
{
#ifdef CAPS_EMUL
    const int dev = 0;
#else
    int dev = 0;
    CAPS_HIP(hipGetDevice(&dev));
#endif
    thread_local std::vector<uint64_t*> words;
    if ((size_t)dev >= words.size()) words.resize((size_t)dev + 1, nullptr);
    if (!words[dev]) words[dev] = static_cast<uint64_t*>(be.alloc(sizeof(uint64_t)));
    return words[dev];
}

// BWT of a slice of a suffix array in HBM (include/caps_sa_hip.h caps_sa_hip_bwt_device_*)
template <typename idx_t>
int bwt_device(const void* dT, uint64_t n, const void* dSA, uint64_t first, uint64_t cnt, void* dBWT, void* stream, uint64_t* primary)
{
    if (!primary) return fail(CAPS_SA_EINVAL, "null primary");
    *primary = ~0ull;
    if (int rc = check_common<idx_t>(dT, n, 0)) return rc;
    if (first > n || cnt > n - first) return fail(CAPS_SA_EINVAL, "first + cnt > n");
    if (cnt == 0) return CAPS_SA_OK;
    if (!dSA || !dBWT) return fail(CAPS_SA_EINVAL, "null pointer");
    return guarded([&]() -> int {
        Backend be(static_cast<decltype(Backend::stream)>(stream));
        uint64_t* dprimary = primary_word(be);
        be.memset(dprimary, 0xFF, sizeof(uint64_t));
        launch_bwt<idx_t>(be, static_cast<const uint8_t*>(dT), n, static_cast<const idx_t*>(dSA), first, cnt, static_cast<uint8_t*>(dBWT),
                          dprimary);
        be.d2h(primary, dprimary, sizeof(uint64_t));
        be.sync();
        return CAPS_SA_OK;
    });
}

// ---- inverse BWT (include/caps_sa_hip.h caps_sa_hip_inverse_bwt_*; kernels.h ibwt_*) ----------------------------------------------
// The workspace: the LF table ((n + 1) entries), the per-tile key counts, C and the range table, then per level of the splitter
// lists succ / len / off (level 0: one node per IBWT_S0 rows; level k + 1: one per IBWT_S1 nodes of level k, until a level has at
// most IBWT_TOP nodes), and the result words of the top walk.
struct IbwtLevels {
    uint32_t levels = 0;
    uint64_t M[16] = {};                                   // nodes of every level
    size_t succ[16] = {}, len[16] = {}, off[16] = {};      // offsets of the level's three lists
};
// the levels over n rows, laid out from offset o on; -> the offset behind the last list
inline size_t ibwt_levels(IbwtLevels& lv, uint64_t n, size_t idx_bytes, size_t o)
{
    for (uint64_t m = n / IBWT_S0 + 1;; m = (m - 1) / IBWT_S1 + 1) {
        lv.M[lv.levels] = m;
        lv.succ[lv.levels] = o; o += align_up(m * idx_bytes);
        lv.len[lv.levels] = o;  o += align_up(m * sizeof(uint64_t));
        lv.off[lv.levels] = o;  o += align_up(m * sizeof(uint64_t));
        ++lv.levels;
        if (m <= IBWT_TOP) return o;
    }
}
struct InvPlan {
    uint64_t n_tiles = 0;
    size_t off_cnt = 0, off_total = 0, off_C = 0, off_sym = 0, off_res = 0;
    IbwtLevels lv;
    size_t bytes = 0;
};
template <typename idx_t> InvPlan inv_plan(uint64_t n)
{
    InvPlan p;
    p.n_tiles = (n + 1 + IBWT_TILE - 1) / IBWT_TILE;
    size_t o = align_up((n + 1) * sizeof(idx_t));
    p.off_cnt = o;   o += align_up(p.n_tiles * IBWT_KEYS * sizeof(idx_t));
    p.off_total = o; o += align_up(IBWT_KEYS * sizeof(uint64_t));
    p.off_C = o;     o += align_up((IBWT_KEYS + 1) * sizeof(uint64_t));
    p.off_sym = o;   o += align_up((IBWT_KEYS + 1) * sizeof(uint64_t));
    p.off_res = o;   o += WS_ALIGN;
    p.bytes = ibwt_levels(p.lv, n, sizeof(idx_t), o);
    return p;
}

inline int inverse_bwt_workspace_bytes(uint64_t n, int idx_bytes, uint64_t* bytes)
{
    if (int rc = check_size_query(n, idx_bytes, bytes, false)) return rc;
    *bytes = ws_reported(idx_bytes == 4 ? inv_plan<uint32_t>(n).bytes : inv_plan<uint64_t>(n).bytes);
    return CAPS_SA_OK;
}

// the kernels on be's stream; the single-cycle check is read back (synchronises): false = not the BWT of any text
template <typename idx_t>
bool run_inverse_bwt(Backend& be, const uint8_t* dB, uint64_t n, uint64_t primary, uint8_t* dT, char* base, const InvPlan& p)
{
    idx_t* LF = reinterpret_cast<idx_t*>(base);
    idx_t* cnt = reinterpret_cast<idx_t*>(base + p.off_cnt);
    uint64_t* total = reinterpret_cast<uint64_t*>(base + p.off_total);
    uint64_t* C = reinterpret_cast<uint64_t*>(base + p.off_C);
    uint64_t* sym = reinterpret_cast<uint64_t*>(base + p.off_sym);
    uint64_t* res = reinterpret_cast<uint64_t*>(base + p.off_res);
    auto succ = [&](uint32_t k) { return reinterpret_cast<idx_t*>(base + p.lv.succ[k]); };
    auto len = [&](uint32_t k) { return reinterpret_cast<uint64_t*>(base + p.lv.len[k]); };
    auto off = [&](uint32_t k) { return reinterpret_cast<uint64_t*>(base + p.lv.off[k]); };
    auto walk_grid = [](uint64_t walks) { return capped_grid(std::min<uint64_t>((walks + IBWT_Q - 1) / IBWT_Q, 8192), IBWT_NT); };
    const uint32_t tg = capped_grid(std::min<uint64_t>(p.n_tiles, 8192), IBWT_NT);
    CAPS_LAUNCH((ibwt_count_kernel<idx_t>), tg, IBWT_NT, be, dB, n, primary, p.n_tiles, cnt);
    CAPS_LAUNCH((ibwt_scan_kernel<idx_t>), IBWT_KEYS, IBWT_NT, be, cnt, p.n_tiles, total);
    CAPS_LAUNCH(ibwt_c_kernel, 1, 64, be, total, C, sym);
    CAPS_LAUNCH((ibwt_lf_kernel<idx_t>), tg, IBWT_NT, be, dB, n, primary, p.n_tiles, cnt, C, LF);
    const uint32_t top = p.lv.levels - 1;
    CAPS_LAUNCH((ibwt_walk_kernel<idx_t, IBWT_LINK0>), walk_grid(p.lv.M[0]), IBWT_NT, be, LF, n, p.lv.M[0], (uint64_t)0,
                (const idx_t*)nullptr, (const uint64_t*)nullptr, (uint64_t*)nullptr, succ(0), len(0), (const uint64_t*)nullptr,
                (const uint64_t*)nullptr, (uint8_t*)nullptr);
    for (uint32_t k = 1; k <= top; ++k)
        CAPS_LAUNCH((ibwt_walk_kernel<idx_t, IBWT_LINK>), walk_grid(p.lv.M[k]), IBWT_NT, be, LF, n, p.lv.M[k], p.lv.M[k - 1],
                    (const idx_t*)succ(k - 1), (const uint64_t*)len(k - 1), (uint64_t*)nullptr, succ(k), len(k),
                    (const uint64_t*)nullptr, (const uint64_t*)nullptr, (uint8_t*)nullptr);
    CAPS_LAUNCH((ibwt_top_kernel<idx_t>), 1, IBWT_NT, be, (const idx_t*)succ(top), (const uint64_t*)len(top), p.lv.M[top], n, off(top), res);
    uint64_t h[3] = {0, 0, 0};
    be.d2h(h, res, sizeof h);
    be.sync();
    if (h[0] != 1) return false;
    for (uint32_t k = top; k >= 1; --k)
        CAPS_LAUNCH((ibwt_walk_kernel<idx_t, IBWT_PROP>), walk_grid(p.lv.M[k]), IBWT_NT, be, LF, n, p.lv.M[k], p.lv.M[k - 1],
                    (const idx_t*)succ(k - 1), (const uint64_t*)len(k - 1), off(k - 1), (idx_t*)nullptr, (uint64_t*)nullptr,
                    (const uint64_t*)off(k), (const uint64_t*)nullptr, (uint8_t*)nullptr);
    CAPS_LAUNCH((ibwt_walk_kernel<idx_t, IBWT_WRITE>), walk_grid(p.lv.M[0]), IBWT_NT, be, LF, n, p.lv.M[0], (uint64_t)0,
                (const idx_t*)nullptr, (const uint64_t*)nullptr, (uint64_t*)nullptr, (idx_t*)nullptr, len(0),
                (const uint64_t*)off(0), (const uint64_t*)sym, dT);
    be.sync();
    return true;
}

inline const char* not_a_bwt_msg() { return "(BWT, primary) is not the BWT of any text: its LF mapping is not one cycle of n + 1 rows"; }

template <typename idx_t> int check_inverse(const void* B, uint64_t n, uint64_t primary, const void* T)
{
    if (n > (uint64_t)std::numeric_limits<idx_t>::max()) return fail(CAPS_SA_EINVAL, "n does not fit 32-bit indices (use the _u64 entry point)");
    if (!B || !T) return fail(CAPS_SA_EINVAL, "null pointer");
    if (primary >= n) return fail(CAPS_SA_EINVAL, "primary >= n");
    return CAPS_SA_OK;
}

// T back from (BWT, primary), device buffers (include/caps_sa_hip.h caps_sa_hip_inverse_bwt_device_*)
template <typename idx_t>
int inverse_bwt_device(const void* dB, uint64_t n, uint64_t primary, void* dT, void* workspace, uint64_t workspace_bytes, void* stream)
{
    if (n == 0) return CAPS_SA_OK;
    if (int rc = check_inverse<idx_t>(dB, n, primary, dT)) return rc;
    if (!workspace) return fail(CAPS_SA_EINVAL, "null workspace");
    const InvPlan p = inv_plan<idx_t>(n);
    if (int rc = ws_check(workspace, workspace_bytes, p.bytes, "workspace too small (caps_sa_hip_inverse_bwt_workspace_bytes)", WS_STRICT)) return rc;
    return guarded([&]() -> int {
        Backend be(static_cast<decltype(Backend::stream)>(stream));
        char* base = align_up(static_cast<char*>(workspace));
        if (!run_inverse_bwt<idx_t>(be, static_cast<const uint8_t*>(dB), n, primary, static_cast<uint8_t*>(dT), base, p))
            return fail(CAPS_SA_EINVAL, not_a_bwt_msg());
        return CAPS_SA_OK;
    });
}

// host buffers: the BWT up, the inverse on the host-path block (HostPathCache), T down
template <typename idx_t>
int inverse_bwt_host(const uint8_t* B, uint64_t n, uint64_t primary, char* T, int device)
{
    if (n == 0) return CAPS_SA_OK;
    if (int rc = check_inverse<idx_t>(B, n, primary, T)) return rc;
    DeviceScope restore_device_;
    if (int rc = set_device(device)) return rc;
    return guarded([&]() -> int {
        HostPathCache& hc = host_cache();
        std::lock_guard<std::mutex> lock(hc.mu);
        Backend be(nullptr);
        hc.blob_host = nullptr;
        const InvPlan p = inv_plan<idx_t>(n);
        const size_t off_T = align_up(n), off_ws = off_T + align_up(n), total = off_ws + p.bytes;
        host_block(hc, be, device, total);
        uint8_t* dB = reinterpret_cast<uint8_t*>(hc.base);
        uint8_t* dT = reinterpret_cast<uint8_t*>(hc.base + off_T);
        be.h2d(dB, B, n);
        if (!run_inverse_bwt<idx_t>(be, dB, n, primary, dT, hc.base + off_ws, p)) return fail(CAPS_SA_EINVAL, not_a_bwt_msg());
        be.d2h(T, dT, n);
        be.sync();
        return CAPS_SA_OK;
    });
}

// ---- FM-index (include/caps_sa_hip.h caps_sa_hip_fm_*; kernels.h fm_*) ------------------------------------------------------------
// The blob: a header of FM_HDR_WORDS 64-bit words, the Occ blocks, then (with samples) the per-block mark ranks and the samples.
constexpr uint64_t FM_MAGIC = 0x31494D4653504143ull;      // "CAPSFMI1"
constexpr uint64_t FM_VERSION = 1, FM_VERSION_TEXT = 2;    // 2: version 1 with samples + the text-position samples behind it
constexpr uint32_t FM_HDR_WORDS = 32;
enum { FMH_MAGIC = 0, FMH_VERSION, FMH_N, FMH_PRIMARY, FMH_IDX_BYTES, FMH_SIGMA, FMH_SYMS, FMH_C0, FMH_S = FMH_C0 + 5, FMH_NSAMPLES,
       FMH_NBLOCKS, FMH_OFF_OCC, FMH_OFF_MRANK, FMH_OFF_SAMPLES, FMH_TOTAL, FMH_T, FMH_NTEXT, FMH_OFF_ROWOF, FMH_TOTAL2 };

// (the sections behind the Occ blocks start at multiples of 64 bytes: part of the blob format, not the workspaces' WS_ALIGN)
inline uint64_t fm_blob_up(uint64_t b) { return (b + 63) & ~uint64_t(63); }
struct FmLayout {
    uint64_t n_blocks = 0, n_samples = 0, off_occ = 0, off_mrank = 0, off_samples = 0, total = 0;
};
inline FmLayout fm_layout(uint64_t n, uint32_t s, int idx_bytes)
{
    const uint64_t rows = idx_bytes == 4 ? 128 : 256, block_bytes = rows / 2;
    FmLayout l;
    l.n_blocks = (n + 1) / rows + 1;
    l.n_samples = s && n ? (n - 1) / s + 1 : 0;
    l.off_occ = FM_HDR_WORDS * sizeof(uint64_t);
    l.off_mrank = l.off_occ + l.n_blocks * block_bytes;
    l.off_samples = l.off_mrank + (s ? fm_blob_up(l.n_blocks * (uint64_t)idx_bytes) : 0);
    l.total = l.off_samples + (s ? fm_blob_up(l.n_samples * (uint64_t)idx_bytes) : 0);
    return l;
}
inline bool fm_sample_ok(uint64_t s) { return s >= 1 && s <= FM_MAX_SAMPLE && (s & (s - 1)) == 0; }
// version 2: rowof[m] behind the version-1 sections, one row per t text positions
struct FmTextLayout {
    uint64_t m = 0, off = 0, total = 0;
};
inline FmTextLayout fm_text_layout(const FmLayout& l, uint64_t n, uint64_t t, int idx_bytes)
{
    FmTextLayout tl;
    tl.m = n ? (n - 1) / t + 1 : 0;
    tl.off = l.total;
    tl.total = tl.off + fm_blob_up(tl.m * (uint64_t)idx_bytes);
    return tl;
}
// the bytes of the blob whose (checked) header is h
inline uint64_t fm_blob_bytes(const uint64_t* h) { return h[FMH_VERSION] == FM_VERSION_TEXT ? h[FMH_TOTAL2] : h[FMH_TOTAL]; }

inline int fm_index_bytes(uint64_t n, uint32_t s, int idx_bytes, uint64_t* bytes)
{
    if (int rc = check_size_query(n, idx_bytes, bytes, false)) return rc;
    if (s && !fm_sample_ok(s)) return fail(CAPS_SA_EINVAL, "sa_sample must be 0 (no samples) or a power of two in 1 .. 1024");
    *bytes = fm_layout(n, s, idx_bytes).total;
    return CAPS_SA_OK;
}
inline int fm_index_bytes_ex(uint64_t n, uint32_t s, uint32_t t, int idx_bytes, uint64_t* bytes)
{
    if (int rc = check_size_query(n, idx_bytes, bytes, false)) return rc;
    if (!fm_sample_ok(s)) return fail(CAPS_SA_EINVAL, "sa_sample must be a power of two in 1 .. 1024 (text samples need SA samples)");
    if (!fm_sample_ok(t) || t < s) return fail(CAPS_SA_EINVAL, "text_sample must be a power of two in sa_sample .. 1024");
    *bytes = fm_text_layout(fm_layout(n, s, idx_bytes), n, t, idx_bytes).total;
    return CAPS_SA_OK;
}

// a few device words of a call (flags, totals), one set per thread and device, kept (primary_word's reasons)
inline uint64_t* call_words(Backend& be)
{
#ifdef CAPS_EMUL
    const int dev = 0;
#else
    int dev = 0;
    CAPS_HIP(hipGetDevice(&dev));
#endif
    thread_local std::vector<uint64_t*> words;
    if ((size_t)dev >= words.size()) words.resize((size_t)dev + 1, nullptr);
    if (!words[dev]) words[dev] = static_cast<uint64_t*>(be.alloc(16 * sizeof(uint64_t)));
    return words[dev];
}

// the header, checked on the host before any kernel reads the body; fills the kernels' view of the blob at dIndex
inline int fm_check_header(const uint64_t* h, uint64_t index_bytes, const void* dIndex, FmView& v)
{
    if (h[FMH_MAGIC] != FM_MAGIC) return fail(CAPS_SA_EINVAL, "not an FM-index of this library (wrong magic)");
    if (h[FMH_VERSION] != FM_VERSION && h[FMH_VERSION] != FM_VERSION_TEXT) return fail(CAPS_SA_EINVAL, "FM-index of another format version");
    const uint64_t ib = h[FMH_IDX_BYTES], n = h[FMH_N], s = h[FMH_S];
    if (ib != 4 && ib != 8) return fail(CAPS_SA_EINVAL, "FM-index header: bad index width");
    if (ib == 4 && n > 0xFFFFFFFFull) return fail(CAPS_SA_EINVAL, "FM-index header: n does not fit its index width");
    if (n >= 1 && h[FMH_PRIMARY] >= n) return fail(CAPS_SA_EINVAL, "FM-index header: primary >= n");
    if (s && !fm_sample_ok(s)) return fail(CAPS_SA_EINVAL, "FM-index header: bad sample distance");
    if (h[FMH_SIGMA] > 4 || (n >= 1 && h[FMH_SIGMA] == 0)) return fail(CAPS_SA_EINVAL, "FM-index header: bad alphabet size");
    const FmLayout l = fm_layout(n, (uint32_t)s, (int)ib);
    if (h[FMH_NBLOCKS] != l.n_blocks || h[FMH_OFF_OCC] != l.off_occ || h[FMH_OFF_MRANK] != l.off_mrank ||
        h[FMH_OFF_SAMPLES] != l.off_samples || h[FMH_TOTAL] != l.total || h[FMH_NSAMPLES] != l.n_samples)
        return fail(CAPS_SA_EINVAL, "FM-index header: section offsets do not fit n, the index width and the sample distance");
    if (l.total > index_bytes) return fail(CAPS_SA_EINVAL, "index_bytes is smaller than the FM-index (truncated blob)");
    if (h[FMH_C0] != 1 || h[FMH_C0 + 4] != n + 1) return fail(CAPS_SA_EINVAL, "FM-index header: bad C[]");
    for (int c = 0; c < 4; ++c)
        if (h[FMH_C0 + c] > h[FMH_C0 + c + 1]) return fail(CAPS_SA_EINVAL, "FM-index header: bad C[]");
    v.n = n;
    v.primary = h[FMH_PRIMARY];
    for (int c = 0; c < 5; ++c) v.C[c] = h[FMH_C0 + c];
    v.n_blocks = l.n_blocks;
    v.n_samples = l.n_samples;
    const char* base = static_cast<const char*>(dIndex);
    v.occ = reinterpret_cast<const uint32_t*>(base + l.off_occ);
    v.mrank = base + l.off_mrank;
    v.samples = base + l.off_samples;
    v.sigma = (uint32_t)h[FMH_SIGMA];
    v.syms = (uint32_t)h[FMH_SYMS];
    v.s = (uint32_t)s;
    v.rowof = nullptr;
    v.n_text_samples = 0;
    v.t = 0;
    if (h[FMH_VERSION] == FM_VERSION_TEXT) {
        const uint64_t t = h[FMH_T];
        if (!s || !fm_sample_ok(t) || t < s) return fail(CAPS_SA_EINVAL, "FM-index header: bad text sample distance");
        const FmTextLayout tl = fm_text_layout(l, n, t, (int)ib);
        if (h[FMH_NTEXT] != tl.m || h[FMH_OFF_ROWOF] != tl.off || h[FMH_TOTAL2] != tl.total)
            return fail(CAPS_SA_EINVAL, "FM-index header: the text-sample section does not fit n, the index width and the sample distances");
        if (tl.total > index_bytes) return fail(CAPS_SA_EINVAL, "index_bytes is smaller than the FM-index (truncated blob)");
        v.rowof = base + tl.off;
        v.n_text_samples = tl.m;
        v.t = (uint32_t)t;
    }
    return CAPS_SA_OK;
}

template <typename idx_t>
int fm_check_build(const void* B, uint64_t n, uint64_t primary, const void* SA, uint64_t s, const void* index, uint64_t index_bytes, uint64_t* need)
{
    if (n > (uint64_t)std::numeric_limits<idx_t>::max()) return fail(CAPS_SA_EINVAL, "n does not fit 32-bit indices (use the _u64 entry point)");
    if (SA && !fm_sample_ok(s)) return fail(CAPS_SA_EINVAL, "sa_sample must be a power of two in 1 .. 1024");
    if (!index) return fail(CAPS_SA_EINVAL, "null index");
    if (n && !B) return fail(CAPS_SA_EINVAL, "null BWT");
    if (n && primary >= n) return fail(CAPS_SA_EINVAL, "primary >= n");
    *need = fm_layout(n, SA ? (uint32_t)s : 0u, (int)sizeof(idx_t)).total;
    if (index_bytes < *need) return fail(CAPS_SA_EINVAL, "index_bytes too small (caps_sa_hip_fm_index_bytes)");
    return CAPS_SA_OK;
}

// the header of (n, primary, s) before the alphabet and C[] are known
template <typename idx_t> void fm_header_init(uint64_t* h, uint64_t n, uint64_t primary, uint32_t s, const FmLayout& l)
{
    std::memset(h, 0, FM_HDR_WORDS * sizeof(uint64_t));
    h[FMH_MAGIC] = FM_MAGIC; h[FMH_VERSION] = FM_VERSION; h[FMH_N] = n; h[FMH_PRIMARY] = n ? primary : 0; h[FMH_IDX_BYTES] = sizeof(idx_t);
    h[FMH_S] = s; h[FMH_NSAMPLES] = l.n_samples; h[FMH_NBLOCKS] = l.n_blocks; h[FMH_OFF_OCC] = l.off_occ; h[FMH_OFF_MRANK] = l.off_mrank;
    h[FMH_OFF_SAMPLES] = l.off_samples; h[FMH_TOTAL] = l.total;
    h[FMH_C0] = 1;
    for (int c = 1; c < 5; ++c) h[FMH_C0 + c] = n + 1;
}
template <typename idx_t> uint64_t fm_tiles(const FmLayout& l) { return (l.n_blocks * FmGeom<idx_t>::ROWS + FM_TILE - 1) / FM_TILE; }

// the device words of a build: the alphabet probe's 8, the tile counts (FM_KEYS columns of n_tiles), the FM_KEYS totals
struct FmScratch {
    uint32_t* present;
    uint64_t *cnt, *total;
};
// n >= 1: the alphabet (read back: synchronises; more than 4 letters is refused before anything is written to the index), then the
// Occ section with zero mark words, and with samples the zero padding of the two sections behind it; the 4 symbol totals are on
// their way to tot[] (the caller synchronises before it reads them)
template <typename idx_t>
int fm_build_occ(Backend& be, const uint8_t* dB, uint64_t n, uint64_t primary, uint32_t s, const FmLayout& l, char* dIndex, const FmScratch& sc,
                 uint64_t* h, uint64_t* tot)
{
    const uint64_t n_tiles = fm_tiles<idx_t>(l);
    be.memset(sc.present, 0, 8 * sizeof(uint32_t));
    CAPS_LAUNCH(fm_probe_kernel, capped_grid(std::min<uint64_t>((n + 16ull * FM_NT - 1) / (16ull * FM_NT), 4096), FM_NT), FM_NT, be, dB, n, sc.present);
    uint32_t pm[8];
    be.d2h(pm, sc.present, sizeof pm);
    be.sync();
    uint32_t sigma = 0, syms = 0;
    for (uint32_t k = 0; k < 256; ++k) {                 // signed-char order: 0x80 .. 0xFF, then 0x00 .. 0x7F
        const uint32_t b = k ^ 0x80u;
        if (!((pm[b / 32] >> (b % 32)) & 1u)) continue;
        if (sigma < 4) syms |= b << (8 * sigma);
        ++sigma;
    }
    if (sigma > 4) return fail(CAPS_SA_EALPHABET, "the BWT has more than 4 distinct bytes: the FM-index packs 2-bit codes (caps_sa_hip_fm_build_wide_* builds the wide index for 1 .. 256)");
    h[FMH_SIGMA] = sigma;
    h[FMH_SYMS] = syms;
    const uint32_t tg = capped_grid(std::min<uint64_t>(n_tiles, 16384), FM_NT);
    CAPS_LAUNCH(fm_tile_count_kernel, tg, FM_NT, be, dB, n, primary, n_tiles, syms, sigma, sc.cnt);
    CAPS_LAUNCH(fm_scan_kernel, 4, FM_NT, be, sc.cnt, n_tiles, 0u, 4u, sc.total);
    uint32_t* occ = reinterpret_cast<uint32_t*>(dIndex + l.off_occ);
    CAPS_LAUNCH((fm_pack_kernel<idx_t>), tg, FM_NT, be, dB, n, primary, n_tiles, l.n_blocks, syms, sigma, (const uint64_t*)sc.cnt, occ);
    be.d2h(tot, sc.total, 4 * sizeof(uint64_t));
    if (s) {
        // (the padding behind the two sections: the blob is the same bytes whatever the memory held)
        const uint64_t mrank_end = l.off_mrank + l.n_blocks * sizeof(idx_t), samples_end = l.off_samples + l.n_samples * sizeof(idx_t);
        if (l.off_samples > mrank_end) be.memset(dIndex + mrank_end, 0, l.off_samples - mrank_end);
        if (l.total > samples_end) be.memset(dIndex + samples_end, 0, l.total - samples_end);
    }
    return CAPS_SA_OK;
}
// C[] into the header from the 4 totals (code 0 also counted the '$' row and the rows behind n)
template <typename idx_t> void fm_header_counts(uint64_t* h, uint64_t* tot, uint64_t n, const FmLayout& l)
{
    const uint64_t pad = fm_tiles<idx_t>(l) * FM_TILE - (n + 1);
    if (tot[0] < pad + 1 || tot[0] - pad - 1 + tot[1] + tot[2] + tot[3] != n) throw HipError("fm build: the symbol counts do not add up to n");
    tot[0] -= pad + 1;
    for (int c = 0; c < 4; ++c) h[FMH_C0 + c + 1] = h[FMH_C0 + c] + tot[c];
}

// the build on be's stream; synchronises (the alphabet and the totals are read back).  hdr_out: the header as written.
template <typename idx_t>
int run_fm_build(Backend& be, const uint8_t* dB, uint64_t n, uint64_t primary, const idx_t* dSA, uint32_t s, char* dIndex, uint64_t* hdr_out)
{
    if (!dSA) s = 0;
    const FmLayout l = fm_layout(n, s, (int)sizeof(idx_t));
    uint64_t h[FM_HDR_WORDS];
    fm_header_init<idx_t>(h, n, primary, s, l);
    if (n == 0) {
        be.memset(dIndex + l.off_occ, 0, l.total - l.off_occ);
    } else {
        DevAllocs da(be);
        const uint64_t n_tiles = fm_tiles<idx_t>(l);
        FmScratch sc;
        sc.present = da.get<uint32_t>(8);
        sc.cnt = da.get<uint64_t>(FM_KEYS * n_tiles);
        sc.total = da.get<uint64_t>(FM_KEYS);
        uint64_t tot[FM_KEYS] = {};
        if (int rc = fm_build_occ<idx_t>(be, dB, n, primary, s, l, dIndex, sc, h, tot)) return rc;
        if (s) {
            const uint32_t tg = capped_grid(std::min<uint64_t>(n_tiles, 16384), FM_NT);
            uint32_t* occ = reinterpret_cast<uint32_t*>(dIndex + l.off_occ);
            idx_t* mrank = reinterpret_cast<idx_t*>(dIndex + l.off_mrank);
            idx_t* samples = reinterpret_cast<idx_t*>(dIndex + l.off_samples);
            CAPS_LAUNCH((fm_mark_kernel<idx_t>), tg, FM_NT, be, dSA, n, n_tiles, l.n_blocks, s, occ, mrank, sc.cnt);
            CAPS_LAUNCH(fm_scan_kernel, 1, FM_NT, be, sc.cnt, n_tiles, 4u, 1u, sc.total);
            CAPS_LAUNCH((fm_sample_kernel<idx_t>), tg, FM_NT, be, dSA, n, n_tiles, l.n_blocks, s, (const uint32_t*)occ, mrank,
                        (const uint64_t*)sc.cnt, samples, l.n_samples);
            be.d2h(tot + 4, sc.total + 4, sizeof(uint64_t));
        }
        be.sync();
        fm_header_counts<idx_t>(h, tot, n, l);
        if (s && tot[4] != l.n_samples)
            return fail(CAPS_SA_EINVAL, ("SA is not the suffix array of a text of n symbols: it holds " + std::to_string(tot[4]) + " multiples of sa_sample, a suffix array " +
                                         std::to_string(l.n_samples)).c_str());
    }
    be.h2d(dIndex, h, sizeof h);
    be.sync();
    if (hdr_out) std::memcpy(hdr_out, h, sizeof h);
    return CAPS_SA_OK;
}

template <typename idx_t>
int fm_build_device(const void* dB, uint64_t n, uint64_t primary, const void* dSA, uint64_t s, void* dIndex, uint64_t index_bytes, void* stream)
{
    uint64_t need = 0;
    if (int rc = fm_check_build<idx_t>(dB, n, primary, dSA, s, dIndex, index_bytes, &need)) return rc;
    return guarded([&]() -> int {
        Backend be(static_cast<decltype(Backend::stream)>(stream));
        return run_fm_build<idx_t>(be, static_cast<const uint8_t*>(dB), n, primary, static_cast<const idx_t*>(dSA), (uint32_t)s,
                                   static_cast<char*>(dIndex), nullptr);
    });
}

// what identifies an uploaded blob beside its address and size: its header and a sum over at most 4096 words of its body
inline uint64_t blob_body_sum(const void* index, uint64_t bytes)
{
    const uint64_t words = bytes / 8, step = std::max<uint64_t>(1, words / 4096);
    uint64_t s = 0, w = 0;
    for (uint64_t k = FM_HDR_WORDS; k < words; k += step) { std::memcpy(&w, static_cast<const char*>(index) + k * 8, 8); s = s * 0x9E3779B97F4A7C15ull + w; }
    return s;
}
inline void blob_mark_resident(HostPathCache& hc, const void* index, uint64_t bytes)
{
    hc.blob_host = index;
    hc.blob_bytes = bytes;
    std::memcpy(hc.blob_hdr, index, sizeof hc.blob_hdr);
    hc.blob_sum = blob_body_sum(index, bytes);
}

template <typename idx_t>
int fm_build_host(const uint8_t* B, uint64_t n, uint64_t primary, const idx_t* SA, uint64_t s, void* index, uint64_t index_bytes, int device)
{
    uint64_t need = 0;
    if (int rc = fm_check_build<idx_t>(B, n, primary, SA, s, index, index_bytes, &need)) return rc;
    DeviceScope restore_device_;
    if (int rc = set_device(device)) return rc;
    return guarded([&]() -> int {
        HostPathCache& hc = host_cache();
        std::lock_guard<std::mutex> lock(hc.mu);
        Backend be(nullptr);
        hc.blob_host = nullptr;
        const size_t off_B = align_up(need), off_SA = off_B + align_up(n ? n : 1), total = off_SA + (SA ? align_up(n * sizeof(idx_t)) : 0) + WS_ALIGN;
        host_block(hc, be, device, total);
        uint8_t* dB = reinterpret_cast<uint8_t*>(hc.base + off_B);
        idx_t* dSA = SA ? reinterpret_cast<idx_t*>(hc.base + off_SA) : nullptr;
        be.h2d(dB, B, n);
        if (SA) be.h2d(dSA, SA, n * sizeof(idx_t));
        if (int rc = run_fm_build<idx_t>(be, dB, n, primary, dSA, (uint32_t)s, hc.base, nullptr)) return rc;
        be.d2h(index, hc.base, need);
        be.sync();
        blob_mark_resident(hc, index, need);
        return CAPS_SA_OK;
    });
}

// ---- FM-index from the BWT alone (include/caps_sa_hip.h caps_sa_hip_fm_build_from_bwt_*; kernels.h fm_walk_kernel) ------------------
// The workspace: the words of the Occ build (FmScratch), the result words of the top walk, the staged rows (one per sample) and the
// inverse BWT's splitter lists (inv_plan's levels: succ / len / off per node).  No array of n entries: n_samples entries of the
// index width + 20 or 24 bytes per IBWT_S0 rows (+ 1/63 of that for the levels above) + 40 bytes per tile.
struct FmBwtPlan {
    size_t off_present = 0, off_cnt = 0, off_total = 0, off_res = 0, off_stage = 0;
    IbwtLevels lv;
    size_t bytes = 0;
};
template <typename idx_t> FmBwtPlan fm_bwt_plan(uint64_t n, uint32_t s)
{
    const FmLayout l = fm_layout(n, s, (int)sizeof(idx_t));
    FmBwtPlan p;
    size_t o = 0;
    p.off_present = o; o += WS_ALIGN;
    p.off_total = o;   o += WS_ALIGN;
    p.off_res = o;     o += WS_ALIGN;
    p.off_cnt = o;     o += align_up(FM_KEYS * fm_tiles<idx_t>(l) * sizeof(uint64_t));
    p.off_stage = o;   o += align_up(l.n_samples * sizeof(idx_t));
    p.bytes = ibwt_levels(p.lv, n, sizeof(idx_t), o);
    return p;
}

inline int fm_from_bwt_workspace_bytes(uint64_t n, uint32_t s, int idx_bytes, uint64_t* bytes)
{
    if (int rc = check_size_query(n, idx_bytes, bytes, false)) return rc;
    if (!fm_sample_ok(s)) return fail(CAPS_SA_EINVAL, "sa_sample must be a power of two in 1 .. 1024");
    *bytes = ws_reported(idx_bytes == 4 ? fm_bwt_plan<uint32_t>(n, s).bytes : fm_bwt_plan<uint64_t>(n, s).bytes);
    return CAPS_SA_OK;
}

template <typename idx_t>
int fm_check_from_bwt(const void* B, uint64_t n, uint64_t primary, uint64_t s, const void* index, uint64_t index_bytes, uint64_t* need)
{
    if (n > (uint64_t)std::numeric_limits<idx_t>::max()) return fail(CAPS_SA_EINVAL, "n does not fit 32-bit indices (use the _u64 entry point)");
    if (s == 0)
        return fail(CAPS_SA_EINVAL, "sa_sample must be a power of two in 1 .. 1024 (an index without samples: caps_sa_hip_fm_build_* with a null SA)");
    if (!fm_sample_ok(s)) return fail(CAPS_SA_EINVAL, "sa_sample must be a power of two in 1 .. 1024");
    if (!index) return fail(CAPS_SA_EINVAL, "null index");
    if (n && !B) return fail(CAPS_SA_EINVAL, "null BWT");
    if (n && primary >= n) return fail(CAPS_SA_EINVAL, "primary >= n");
    *need = fm_layout(n, (uint32_t)s, (int)sizeof(idx_t)).total;
    if (index_bytes < *need) return fail(CAPS_SA_EINVAL, "index_bytes too small (caps_sa_hip_fm_index_bytes)");
    return CAPS_SA_OK;
}

// the build on be's stream, workspace at base (256-byte aligned); synchronises (alphabet, totals, the single-cycle check)
template <typename idx_t>
int run_fm_from_bwt(Backend& be, const uint8_t* dB, uint64_t n, uint64_t primary, uint32_t s, char* dIndex, char* base, const FmBwtPlan& p)
{
    const FmLayout l = fm_layout(n, s, (int)sizeof(idx_t));
    uint64_t h[FM_HDR_WORDS];
    fm_header_init<idx_t>(h, n, primary, s, l);
    if (n == 0) {
        be.memset(dIndex + l.off_occ, 0, l.total - l.off_occ);
    } else {
        const uint64_t n_tiles = fm_tiles<idx_t>(l);
        FmScratch sc;
        sc.present = reinterpret_cast<uint32_t*>(base + p.off_present);
        sc.cnt = reinterpret_cast<uint64_t*>(base + p.off_cnt);
        sc.total = reinterpret_cast<uint64_t*>(base + p.off_total);
        uint64_t* res = reinterpret_cast<uint64_t*>(base + p.off_res);
        idx_t* stage = reinterpret_cast<idx_t*>(base + p.off_stage);
        auto succ = [&](uint32_t k) { return reinterpret_cast<idx_t*>(base + p.lv.succ[k]); };
        auto len = [&](uint32_t k) { return reinterpret_cast<uint64_t*>(base + p.lv.len[k]); };
        auto off = [&](uint32_t k) { return reinterpret_cast<uint64_t*>(base + p.lv.off[k]); };
        uint64_t tot[FM_KEYS] = {};
        if (int rc = fm_build_occ<idx_t>(be, dB, n, primary, s, l, dIndex, sc, h, tot)) return rc;
        be.sync();
        fm_header_counts<idx_t>(h, tot, n, l);
        FmView v;
        if (int rc = fm_check_header(h, l.total, dIndex, v)) return rc;
        uint32_t* occ = reinterpret_cast<uint32_t*>(dIndex + l.off_occ);
        idx_t* mrank = reinterpret_cast<idx_t*>(dIndex + l.off_mrank);
        idx_t* samples = reinterpret_cast<idx_t*>(dIndex + l.off_samples);
        auto walk_grid = [](uint64_t walks) { return capped_grid(std::min<uint64_t>((walks + IBWT_Q - 1) / IBWT_Q, 8192), IBWT_NT); };
        const uint32_t top = p.lv.levels - 1;
        CAPS_LAUNCH((fm_walk_kernel<idx_t, FMW_LINK0>), walk_grid(p.lv.M[0]), IBWT_NT, be, v, p.lv.M[0], succ(0), len(0), (const uint64_t*)nullptr,
                    (uint32_t*)nullptr, (idx_t*)nullptr);
        // the list levels of the inverse BWT as they are (they never touch LF)
        for (uint32_t k = 1; k <= top; ++k)
            CAPS_LAUNCH((ibwt_walk_kernel<idx_t, IBWT_LINK>), walk_grid(p.lv.M[k]), IBWT_NT, be, (const idx_t*)nullptr, n, p.lv.M[k], p.lv.M[k - 1],
                        (const idx_t*)succ(k - 1), (const uint64_t*)len(k - 1), (uint64_t*)nullptr, succ(k), len(k),
                        (const uint64_t*)nullptr, (const uint64_t*)nullptr, (uint8_t*)nullptr);
        CAPS_LAUNCH((ibwt_top_kernel<idx_t>), 1, IBWT_NT, be, (const idx_t*)succ(top), (const uint64_t*)len(top), p.lv.M[top], n, off(top), res);
        uint64_t flag[3] = {0, 0, 0};
        be.d2h(flag, res, sizeof flag);
        be.sync();
        if (flag[0] != 1) return fail(CAPS_SA_EINVAL, not_a_bwt_msg());
        for (uint32_t k = top; k >= 1; --k)
            CAPS_LAUNCH((ibwt_walk_kernel<idx_t, IBWT_PROP>), walk_grid(p.lv.M[k]), IBWT_NT, be, (const idx_t*)nullptr, n, p.lv.M[k], p.lv.M[k - 1],
                        (const idx_t*)succ(k - 1), (const uint64_t*)len(k - 1), off(k - 1), (idx_t*)nullptr, (uint64_t*)nullptr,
                        (const uint64_t*)off(k), (const uint64_t*)nullptr, (uint8_t*)nullptr);
        CAPS_LAUNCH((fm_walk_kernel<idx_t, FMW_MARK>), walk_grid(p.lv.M[0]), IBWT_NT, be, v, p.lv.M[0], (idx_t*)nullptr, len(0), (const uint64_t*)off(0),
                    occ, stage);
        const uint32_t tg = capped_grid(std::min<uint64_t>(n_tiles, 16384), FM_NT);
        CAPS_LAUNCH((fm_mark_kernel<idx_t, true>), tg, FM_NT, be, (const idx_t*)nullptr, n, n_tiles, l.n_blocks, s, occ, mrank, sc.cnt);
        CAPS_LAUNCH(fm_scan_kernel, 1, FM_NT, be, sc.cnt, n_tiles, 4u, 1u, sc.total);
        CAPS_LAUNCH((fm_mrank_abs_kernel<idx_t>), capped_grid(std::min<uint64_t>((l.n_blocks + FM_NT - 1) / FM_NT, 16384), FM_NT), FM_NT, be, mrank,
                    l.n_blocks, n_tiles, (const uint64_t*)sc.cnt);
        CAPS_LAUNCH((fm_place_kernel<idx_t>), capped_grid(std::min<uint64_t>((l.n_samples + FM_NT - 1) / FM_NT, 1u << 20), FM_NT), FM_NT, be, v,
                    (const idx_t*)stage, samples);
        be.d2h(tot + 4, sc.total + 4, sizeof(uint64_t));
        be.sync();
        if (tot[4] != l.n_samples) throw HipError("fm build from the BWT: the marked rows are not one per sample");
    }
    be.h2d(dIndex, h, sizeof h);
    be.sync();
    return CAPS_SA_OK;
}

template <typename idx_t>
int fm_build_from_bwt_device(const void* dB, uint64_t n, uint64_t primary, uint64_t s, void* dIndex, uint64_t index_bytes, void* workspace,
                             uint64_t workspace_bytes, void* stream)
{
    uint64_t need = 0;
    if (int rc = fm_check_from_bwt<idx_t>(dB, n, primary, s, dIndex, index_bytes, &need)) return rc;
    const FmBwtPlan p = fm_bwt_plan<idx_t>(n, (uint32_t)s);
    if (int rc = ws_check(workspace, workspace_bytes, p.bytes, "workspace too small (caps_sa_hip_fm_from_bwt_workspace_bytes)", WS_STRICT)) return rc;
    return guarded([&]() -> int {
        Backend be(static_cast<decltype(Backend::stream)>(stream));
        DevAllocs da(be);                                    // a null workspace: allocated here, freed on return
        char* base = ws_carve(da, workspace, p.bytes);
        return run_fm_from_bwt<idx_t>(be, static_cast<const uint8_t*>(dB), n, primary, (uint32_t)s, static_cast<char*>(dIndex), base, p);
    });
}

// host buffers: the BWT up, the index built at the head of the host-path block and downloaded; it stays there for the host queries
template <typename idx_t>
int fm_build_from_bwt_host(const uint8_t* B, uint64_t n, uint64_t primary, uint64_t s, void* index, uint64_t index_bytes, int device)
{
    uint64_t need = 0;
    if (int rc = fm_check_from_bwt<idx_t>(B, n, primary, s, index, index_bytes, &need)) return rc;
    DeviceScope restore_device_;
    if (int rc = set_device(device)) return rc;
    return guarded([&]() -> int {
        HostPathCache& hc = host_cache();
        std::lock_guard<std::mutex> lock(hc.mu);
        Backend be(nullptr);
        hc.blob_host = nullptr;
        const FmBwtPlan p = fm_bwt_plan<idx_t>(n, (uint32_t)s);
        const size_t off_B = align_up(need), off_ws = off_B + align_up(n ? n : 1), total = off_ws + p.bytes;
        host_block(hc, be, device, total);
        uint8_t* dB = reinterpret_cast<uint8_t*>(hc.base + off_B);
        be.h2d(dB, B, n);
        if (int rc = run_fm_from_bwt<idx_t>(be, dB, n, primary, (uint32_t)s, hc.base, hc.base + off_ws, p)) return rc;
        be.d2h(index, hc.base, need);
        be.sync();
        blob_mark_resident(hc, index, need);
        return CAPS_SA_OK;
    });
}

// ---- the wide FM-index (include/caps_sa_hip.h "FM-index: the wide format"; kernels.h fmw_*) -----------------------------------------
// header | table section (FMW_TAB_BYTES) | Lv level sections of n_blocks blocks | mark ranks | samples (the last two as in version 1)
constexpr uint64_t FMW_MAGIC = 0x31574D4653504143ull;     // "CAPSFMW1"
constexpr uint64_t FMW_VERSION = 1;
// words 2 .. 4 and 12 .. 18 are version 1's (FMH_*: word 15 = the offset of level 0); the wide format's own:
enum { FMWH_LV = 6, FMWH_OFF_TAB = 7, FMWH_LEVEL_BYTES = 8 };

inline uint32_t fmw_levels(uint64_t sigma)
{
    uint32_t lv = 1;
    while (lv < FMW_MAX_LV && (1ull << (2 * lv)) < sigma) ++lv;
    return lv;
}
struct FmwLayout {
    uint32_t Lv = 1;
    uint64_t n_blocks = 0, n_samples = 0, off_tab = 0, off_lev0 = 0, level_bytes = 0, off_mrank = 0, off_samples = 0, total = 0;
};
inline FmwLayout fmw_layout(uint64_t n, uint64_t sigma, uint32_t s, int idx_bytes)
{
    const uint64_t rows = idx_bytes == 4 ? 128 : 256;
    FmwLayout l;
    l.Lv = fmw_levels(sigma);
    l.n_blocks = (n + 1) / rows + 1;
    l.n_samples = s && n ? (n - 1) / s + 1 : 0;
    l.off_tab = FM_HDR_WORDS * sizeof(uint64_t);
    l.off_lev0 = l.off_tab + FMW_TAB_BYTES;
    l.level_bytes = l.n_blocks * (rows / 2);
    l.off_mrank = l.off_lev0 + l.Lv * l.level_bytes;
    l.off_samples = l.off_mrank + (s ? fm_blob_up(l.n_blocks * (uint64_t)idx_bytes) : 0);
    l.total = l.off_samples + (s ? fm_blob_up(l.n_samples * (uint64_t)idx_bytes) : 0);
    return l;
}
inline int fmw_index_bytes(uint64_t n, uint32_t sigma, uint32_t s, int idx_bytes, uint64_t* bytes)
{
    if (int rc = check_size_query(n, idx_bytes, bytes, false)) return rc;
    if (s && !fm_sample_ok(s)) return fail(CAPS_SA_EINVAL, "sa_sample must be 0 (no samples) or a power of two in 1 .. 1024");
    if (sigma > 256) return fail(CAPS_SA_EINVAL, "sigma must be 0 (unknown) or 1 .. 256");
    *bytes = fmw_layout(n, sigma ? sigma : 256, s, idx_bytes).total;
    return CAPS_SA_OK;
}

// the host's image of the table section
struct FmwTable {
    uint64_t w[FMW_TAB_BYTES / 8];
    FmwTable() { std::memset(w, 0, sizeof w); }
    uint8_t* letters() { return reinterpret_cast<uint8_t*>(w) + FMW_TAB_LETTERS; }
    uint8_t* code_of() { return reinterpret_cast<uint8_t*>(w) + FMW_TAB_CODE; }
    uint64_t* C() { return w + FMW_TAB_C / 8; }
    uint64_t* zone() { return w + FMW_TAB_ZONE / 8; }
    uint64_t* Z() { return w + FMW_TAB_Z / 8; }
};
// letters[] and code_of[] from the byte set (256 bits), in signed-char order; -> sigma
inline uint32_t fmw_alphabet(const uint32_t* present, FmwTable& t)
{
    uint32_t sigma = 0;
    for (uint32_t k = 0; k < 256; ++k) {                 // signed-char order: 0x80 .. 0xFF, then 0x00 .. 0x7F
        const uint32_t b = k ^ 0x80u;
        t.code_of()[b] = (uint8_t)(sigma < 256 ? sigma : 255);     // (the letters below b; 255 letters below 0x7F at most)
        if ((present[b / 32] >> (b % 32)) & 1u) t.letters()[sigma++] = (uint8_t)b;
    }
    return sigma;
}
// zone[] and Z[][] from C[] (n >= 1): K[c] = the rows 0 .. n that store code c -- the letters of code c, and the '$' row with code
// 0.  Level l orders the rows by (digit l - 1, .., digit 0), so code c comes from position 0 to the number of rows whose code has a
// smaller digit-reversed value.
inline void fmw_zones(uint64_t sigma, uint32_t Lv, const uint64_t* C, uint64_t* zone, uint64_t* Z)
{
    uint64_t K[256];
    for (uint32_t c = 0; c < 256; ++c) K[c] = c < sigma ? C[c + 1] - C[c] + (c == 0 ? 1 : 0) : 0;
    // (one pass per table, every call: the codes in digit-reversed order by a 256-entry bucket array, then a running sum)
    uint32_t by_rev[256];
    for (uint32_t r = 0; r < 256; ++r) by_rev[r] = 256;
    for (uint32_t c = 0; c < sigma; ++c) {
        uint32_t r = 0;
        for (uint32_t l = 0; l < Lv; ++l) r = 4 * r + ((c >> (2 * l)) & 3u);
        by_rev[r] = c;
    }
    for (uint32_t c = 0; c < 256; ++c) zone[c] = 0;
    uint64_t below = 0;
    for (uint32_t r = 0; r < 256; ++r)
        if (by_rev[r] < 256) { zone[by_rev[r]] = below; below += K[by_rev[r]]; }
    for (uint32_t i = 0; i < 4 * FMW_MAX_LV; ++i) Z[i] = 0;
    for (uint32_t l = 0; l < Lv; ++l) {
        uint64_t per[4] = {0, 0, 0, 0};
        for (uint32_t k = 0; k < sigma; ++k) per[(k >> (2 * (Lv - 1 - l))) & 3u] += K[k];
        for (uint32_t d = 1; d < 4; ++d) Z[4 * l + d] = Z[4 * l + d - 1] + per[d - 1];
    }
}

// header and table section, checked on the host before any kernel reads the body; fills v (what the shared host code reads: n, s,
// the sample counts) and w (the wide kernels' view of the blob at dIndex)
inline int fmw_check(const uint64_t* h, const uint64_t* tab, uint64_t index_bytes, const void* dIndex, FmView& v, FmwView& w)
{
    if (h[FMH_VERSION] != FMW_VERSION) return fail(CAPS_SA_EINVAL, "wide FM-index of another format version");
    const uint64_t ib = h[FMH_IDX_BYTES], n = h[FMH_N], s = h[FMH_S], sigma = h[FMH_SIGMA];
    if (ib != 4 && ib != 8) return fail(CAPS_SA_EINVAL, "FM-index header: bad index width");
    if (ib == 4 && n > 0xFFFFFFFFull) return fail(CAPS_SA_EINVAL, "FM-index header: n does not fit its index width");
    if (n >= 1 && h[FMH_PRIMARY] >= n) return fail(CAPS_SA_EINVAL, "FM-index header: primary >= n");
    if (s && !fm_sample_ok(s)) return fail(CAPS_SA_EINVAL, "FM-index header: bad sample distance");
    if (sigma > 256 || sigma > n || (n >= 1 && sigma == 0)) return fail(CAPS_SA_EINVAL, "FM-index header: bad alphabet size");
    const FmwLayout l = fmw_layout(n, sigma, (uint32_t)s, (int)ib);
    if (h[FMWH_LV] != l.Lv) return fail(CAPS_SA_EINVAL, "FM-index header: the number of levels does not fit the alphabet size");
    if (h[FMH_NBLOCKS] != l.n_blocks || h[FMWH_OFF_TAB] != l.off_tab || h[FMH_OFF_OCC] != l.off_lev0 || h[FMWH_LEVEL_BYTES] != l.level_bytes ||
        h[FMH_OFF_MRANK] != l.off_mrank || h[FMH_OFF_SAMPLES] != l.off_samples || h[FMH_TOTAL] != l.total || h[FMH_NSAMPLES] != l.n_samples)
        return fail(CAPS_SA_EINVAL, "FM-index header: section offsets do not fit n, the alphabet, the index width and the sample distance");
    if (l.total > index_bytes) return fail(CAPS_SA_EINVAL, "index_bytes is smaller than the FM-index (truncated blob)");
    const uint8_t* letters = reinterpret_cast<const uint8_t*>(tab) + FMW_TAB_LETTERS;
    const uint8_t* code_of = reinterpret_cast<const uint8_t*>(tab) + FMW_TAB_CODE;
    const uint64_t *C = tab + FMW_TAB_C / 8, *zone = tab + FMW_TAB_ZONE / 8, *Z = tab + FMW_TAB_Z / 8;
    {
        uint32_t present[8] = {};
        for (uint64_t c = 0; c < 256; ++c) {
            if (c >= sigma) { if (letters[c]) return fail(CAPS_SA_EINVAL, "FM-index table: bad letters"); continue; }
            if (c && (letters[c] ^ 0x80u) <= (letters[c - 1] ^ 0x80u)) return fail(CAPS_SA_EINVAL, "FM-index table: bad letters");
            present[letters[c] / 32] |= 1u << (letters[c] % 32);
        }
        FmwTable t;
        if (n) fmw_alphabet(present, t);
        if (std::memcmp(t.code_of(), code_of, 256) != 0) return fail(CAPS_SA_EINVAL, "FM-index table: code_of[] does not fit the letters");
    }
    if (C[0] != 1 || C[256] != n + 1) return fail(CAPS_SA_EINVAL, "FM-index table: bad C[]");
    for (uint32_t c = 0; c < 256; ++c)
        if (C[c] > C[c + 1] || (c >= sigma && C[c] != n + 1)) return fail(CAPS_SA_EINVAL, "FM-index table: bad C[]");
    {
        uint64_t zn[256], Zn[4 * FMW_MAX_LV];
        fmw_zones(n ? sigma : 0, l.Lv, C, zn, Zn);
        if (std::memcmp(zn, zone, sizeof zn) != 0) return fail(CAPS_SA_EINVAL, "FM-index table: zone[] does not fit C[]");
        if (std::memcmp(Zn, Z, sizeof Zn) != 0) return fail(CAPS_SA_EINVAL, "FM-index table: Z[][] does not fit C[]");
    }
    const char* base = static_cast<const char*>(dIndex);
    v = FmView{};
    v.n = n;
    v.primary = h[FMH_PRIMARY];
    v.n_blocks = l.n_blocks;
    v.n_samples = l.n_samples;
    v.s = (uint32_t)s;
    w.n = n;
    w.primary = h[FMH_PRIMARY];
    w.n_blocks = l.n_blocks;
    w.n_samples = l.n_samples;
    w.lev_words = l.level_bytes / 4;
    w.lev0 = reinterpret_cast<const uint32_t*>(base + l.off_lev0);
    w.mrank = base + l.off_mrank;
    w.samples = base + l.off_samples;
    w.tab = reinterpret_cast<const uint64_t*>(base + l.off_tab);
    w.sigma = (uint32_t)sigma;
    w.Lv = l.Lv;
    w.s = (uint32_t)s;
    return CAPS_SA_OK;
}
constexpr const char* FMW_NOT_BUILT = "this is a wide FM-index (\"CAPSFMW1\"): text samples and extract are not built for the wide format";

// any blob at dIndex (device memory) whose header h has been read: a narrow one fills v (w.Lv = 0), a wide one has its table
// section read back and checked and fills both
inline int fm_check_any(Backend& be, const uint64_t* h, uint64_t index_bytes, const void* dIndex, FmView& v, FmwView& w)
{
    w = FmwView{};
    if (h[FMH_MAGIC] != FMW_MAGIC) return fm_check_header(h, index_bytes, dIndex, v);
    if (index_bytes < FM_HDR_WORDS * sizeof(uint64_t) + FMW_TAB_BYTES) return fail(CAPS_SA_EINVAL, "index_bytes is smaller than the FM-index (truncated blob)");
    FmwTable t;
    be.d2h(t.w, static_cast<const char*>(dIndex) + FM_HDR_WORDS * sizeof(uint64_t), FMW_TAB_BYTES);
    be.sync();
    return fmw_check(h, t.w, index_bytes, dIndex, v, w);
}

template <typename idx_t>
int fmw_check_build(const void* B, uint64_t n, uint64_t primary, const void* SA, uint64_t s, const void* index, uint64_t index_bytes)
{
    if (n > (uint64_t)std::numeric_limits<idx_t>::max()) return fail(CAPS_SA_EINVAL, "n does not fit 32-bit indices (use the _u64 entry point)");
    if (SA && !fm_sample_ok(s)) return fail(CAPS_SA_EINVAL, "sa_sample must be a power of two in 1 .. 1024");
    if (!index) return fail(CAPS_SA_EINVAL, "null index");
    if (n && !B) return fail(CAPS_SA_EINVAL, "null BWT");
    if (n && primary >= n) return fail(CAPS_SA_EINVAL, "primary >= n");
    // (the alphabet is not known yet: room for the smallest index is asked for here, for the actual one once the letters are counted)
    if (index_bytes < fmw_layout(n, std::min<uint64_t>(n, 1), SA ? (uint32_t)s : 0u, (int)sizeof(idx_t)).total)
        return fail(CAPS_SA_EINVAL, "index_bytes too small (caps_sa_hip_fm_wide_index_bytes)");
    return CAPS_SA_OK;
}

// the workspace: present words | tile counts (FM_KEYS columns) | 256 totals | the code histogram (256 columns of FMW_HIST_WGS) |
// two code buffers of n + 1 bytes (each up to a multiple of 64); every part 256-byte aligned.  No array of n index entries.
constexpr uint32_t FMW_HIST_WGS = 1024;
struct FmwPlan { size_t off_present, off_cnt, off_total, off_hist, off_a, off_b, bytes; uint64_t n_tiles, cap; uint32_t hist_wgs; };
template <typename idx_t> FmwPlan fmw_plan(uint64_t n)
{
    FmwPlan p;
    const uint64_t n_blocks = (n + 1) / FmGeom<idx_t>::ROWS + 1;
    p.n_tiles = (n_blocks * FmGeom<idx_t>::ROWS + FM_TILE - 1) / FM_TILE;
    p.cap = (n + 1 + 63) & ~uint64_t(63);
    p.hist_wgs = (uint32_t)std::min<uint64_t>((n / FM_WROWS + 1 + FM_NT - 1) / FM_NT, FMW_HIST_WGS);
    p.off_present = 0;
    p.off_cnt = align_up(8 * sizeof(uint32_t));
    p.off_total = p.off_cnt + align_up(FM_KEYS * p.n_tiles * sizeof(uint64_t));
    p.off_hist = p.off_total + align_up(256 * sizeof(uint64_t));
    p.off_a = p.off_hist + align_up(256ull * p.hist_wgs * sizeof(uint64_t));
    p.off_b = p.off_a + align_up(p.cap);
    p.bytes = p.off_b + align_up(p.cap);
    return p;
}
inline int fmw_workspace_bytes(uint64_t n, int idx_bytes, uint64_t* bytes)
{
    if (int rc = check_size_query(n, idx_bytes, bytes, false)) return rc;
    *bytes = ws_reported(idx_bytes == 4 ? fmw_plan<uint32_t>(n).bytes : fmw_plan<uint64_t>(n).bytes);
    return CAPS_SA_OK;
}

// the build on be's stream, workspace at base (256-byte aligned); synchronises.  capacity: the bytes at dIndex.
template <typename idx_t>
int run_fmw_build(Backend& be, const uint8_t* dB, uint64_t n, uint64_t primary, const idx_t* dSA, uint32_t s, char* dIndex, uint64_t capacity,
                  char* base, const FmwPlan& p, uint64_t* total_out)
{
    if (!dSA) s = 0;
    uint64_t h[FM_HDR_WORDS];
    std::memset(h, 0, sizeof h);
    FmwTable t;
    uint64_t sigma = 0;
    uint32_t* present = reinterpret_cast<uint32_t*>(base + p.off_present);
    uint64_t* cnt = reinterpret_cast<uint64_t*>(base + p.off_cnt);
    uint64_t* total = reinterpret_cast<uint64_t*>(base + p.off_total);
    uint64_t* hist = reinterpret_cast<uint64_t*>(base + p.off_hist);
    uint8_t* cur = reinterpret_cast<uint8_t*>(base + p.off_a);
    uint8_t* nxt = reinterpret_cast<uint8_t*>(base + p.off_b);
    if (n) {
        be.memset(present, 0, 8 * sizeof(uint32_t));
        CAPS_LAUNCH(fm_probe_kernel, capped_grid(std::min<uint64_t>((n + 16ull * FM_NT - 1) / (16ull * FM_NT), 4096), FM_NT), FM_NT, be, dB, n, present);
        uint32_t pm[8];
        be.d2h(pm, present, sizeof pm);
        be.sync();
        sigma = fmw_alphabet(pm, t);
    }
    const FmwLayout l = fmw_layout(n, sigma, s, (int)sizeof(idx_t));
    if (capacity < l.total)
        return fail(CAPS_SA_EINVAL, ("index_bytes too small: the BWT has " + std::to_string(sigma) + " distinct bytes (caps_sa_hip_fm_wide_index_bytes)").c_str());
    h[FMH_MAGIC] = FMW_MAGIC; h[FMH_VERSION] = FMW_VERSION; h[FMH_N] = n; h[FMH_PRIMARY] = n ? primary : 0; h[FMH_IDX_BYTES] = sizeof(idx_t);
    h[FMH_SIGMA] = sigma; h[FMWH_LV] = l.Lv; h[FMWH_OFF_TAB] = l.off_tab; h[FMWH_LEVEL_BYTES] = l.level_bytes;
    h[FMH_S] = s; h[FMH_NSAMPLES] = l.n_samples; h[FMH_NBLOCKS] = l.n_blocks; h[FMH_OFF_OCC] = l.off_lev0; h[FMH_OFF_MRANK] = l.off_mrank;
    h[FMH_OFF_SAMPLES] = l.off_samples; h[FMH_TOTAL] = l.total;
    uint64_t* C = t.C();
    C[0] = 1;
    for (uint32_t c = 1; c <= 256; ++c) C[c] = n + 1;
    if (n == 0) {
        be.memset(dIndex + l.off_lev0, 0, l.total - l.off_lev0);
    } else {
        // the letters' table is read by the code kernel from its place in the blob
        be.h2d(dIndex + l.off_tab, t.w, FMW_TAB_BYTES);
        CAPS_LAUNCH(fmw_code_kernel, p.hist_wgs, FM_NT, be, dB, n, primary, reinterpret_cast<const uint8_t*>(dIndex + l.off_tab + FMW_TAB_CODE), cur, hist);
        CAPS_LAUNCH(fm_scan_kernel, 256, FM_NT, be, hist, (uint64_t)p.hist_wgs, 0u, 256u, total);
        uint64_t K[256];
        be.d2h(K, total, sizeof K);
        be.sync();
        uint64_t sum = 0;
        for (uint32_t c = 0; c < 256; ++c) sum += K[c];
        if (K[0] == 0 || sum != n + 1) throw HipError("fm wide build: the symbol counts do not add up to n");
        K[0] -= 1;                                           // (the '$' row)
        for (uint32_t c = 0; c < 256; ++c) C[c + 1] = C[c] + K[c];
        fmw_zones(sigma, l.Lv, C, t.zone(), t.Z());
        const uint32_t tg = capped_grid(std::min<uint64_t>(p.n_tiles, 16384), FM_NT);
        for (uint32_t lev = 0; lev < l.Lv; ++lev) {
            const uint32_t shift = 2 * (l.Lv - 1 - lev);
            uint32_t* occ = reinterpret_cast<uint32_t*>(dIndex + l.off_lev0 + lev * l.level_bytes);
            CAPS_LAUNCH(fmw_count_kernel, tg, FM_NT, be, (const uint8_t*)cur, n, p.n_tiles, shift, cnt);
            CAPS_LAUNCH(fm_scan_kernel, 4, FM_NT, be, cnt, p.n_tiles, 0u, 4u, total);
            CAPS_LAUNCH((fmw_pack_kernel<idx_t>), tg, FM_NT, be, (const uint8_t*)cur, n, p.n_tiles, l.n_blocks, shift, (const uint64_t*)cnt, occ);
            if (lev + 1 < l.Lv) {
                const uint64_t* Z = t.Z() + 4 * lev;
                CAPS_LAUNCH(fmw_scatter_kernel, tg, FM_NT, be, (const uint8_t*)cur, nxt, n, p.cap, p.n_tiles, shift, (const uint64_t*)cnt, Z[1], Z[2], Z[3]);
                std::swap(cur, nxt);
            }
        }
        uint64_t marked = 0;
        if (s) {
            const uint64_t mrank_end = l.off_mrank + l.n_blocks * sizeof(idx_t), samples_end = l.off_samples + l.n_samples * sizeof(idx_t);
            if (l.off_samples > mrank_end) be.memset(dIndex + mrank_end, 0, l.off_samples - mrank_end);
            if (l.total > samples_end) be.memset(dIndex + samples_end, 0, l.total - samples_end);
            uint32_t* occ = reinterpret_cast<uint32_t*>(dIndex + l.off_lev0);
            idx_t* mrank = reinterpret_cast<idx_t*>(dIndex + l.off_mrank);
            idx_t* samples = reinterpret_cast<idx_t*>(dIndex + l.off_samples);
            CAPS_LAUNCH((fm_mark_kernel<idx_t>), tg, FM_NT, be, dSA, n, p.n_tiles, l.n_blocks, s, occ, mrank, cnt);
            CAPS_LAUNCH(fm_scan_kernel, 1, FM_NT, be, cnt, p.n_tiles, 4u, 1u, total);
            CAPS_LAUNCH((fm_sample_kernel<idx_t>), tg, FM_NT, be, dSA, n, p.n_tiles, l.n_blocks, s, (const uint32_t*)occ, mrank, (const uint64_t*)cnt, samples,
                        l.n_samples);
            be.d2h(&marked, total + 4, sizeof(uint64_t));
        }
        be.sync();
        if (s && marked != l.n_samples)
            return fail(CAPS_SA_EINVAL, ("SA is not the suffix array of a text of n symbols: it holds " + std::to_string(marked) + " multiples of sa_sample, a suffix array " +
                                         std::to_string(l.n_samples)).c_str());
    }
    be.h2d(dIndex + l.off_tab, t.w, FMW_TAB_BYTES);
    be.h2d(dIndex, h, sizeof h);
    be.sync();
    if (total_out) *total_out = l.total;
    return CAPS_SA_OK;
}

template <typename idx_t>
int fmw_build_device(const void* dB, uint64_t n, uint64_t primary, const void* dSA, uint64_t s, void* dIndex, uint64_t index_bytes, void* workspace,
                     uint64_t workspace_bytes, void* stream)
{
    if (int rc = fmw_check_build<idx_t>(dB, n, primary, dSA, s, dIndex, index_bytes)) return rc;
    const FmwPlan p = fmw_plan<idx_t>(n);
    if (int rc = ws_check(workspace, workspace_bytes, p.bytes, "workspace too small (caps_sa_hip_fm_wide_workspace_bytes)", WS_STRICT)) return rc;
    return guarded([&]() -> int {
        Backend be(static_cast<decltype(Backend::stream)>(stream));
        DevAllocs da(be);                                    // a null workspace: allocated here, freed on return
        char* base = ws_carve(da, workspace, p.bytes);
        return run_fmw_build<idx_t>(be, static_cast<const uint8_t*>(dB), n, primary, static_cast<const idx_t*>(dSA), (uint32_t)s,
                                    static_cast<char*>(dIndex), index_bytes, base, p, nullptr);
    });
}

// host buffers: BWT and SA up, the index built at the head of the host-path block and downloaded; it stays there for the host queries
template <typename idx_t>
int fmw_build_host(const uint8_t* B, uint64_t n, uint64_t primary, const idx_t* SA, uint64_t s, void* index, uint64_t index_bytes, int device)
{
    if (int rc = fmw_check_build<idx_t>(B, n, primary, SA, s, index, index_bytes)) return rc;
    DeviceScope restore_device_;
    if (int rc = set_device(device)) return rc;
    return guarded([&]() -> int {
        HostPathCache& hc = host_cache();
        std::lock_guard<std::mutex> lock(hc.mu);
        Backend be(nullptr);
        hc.blob_host = nullptr;
        const FmwPlan p = fmw_plan<idx_t>(n);
        const uint64_t room = std::min<uint64_t>(index_bytes, fmw_layout(n, 256, SA ? (uint32_t)s : 0u, (int)sizeof(idx_t)).total);
        const size_t off_B = align_up(room), off_SA = off_B + align_up(n ? n : 1), off_ws = off_SA + (SA ? align_up(n * sizeof(idx_t)) : 0),
                     total = off_ws + p.bytes;
        host_block(hc, be, device, total);
        uint8_t* dB = reinterpret_cast<uint8_t*>(hc.base + off_B);
        idx_t* dSA = SA ? reinterpret_cast<idx_t*>(hc.base + off_SA) : nullptr;
        be.h2d(dB, B, n);
        if (SA) be.h2d(dSA, SA, n * sizeof(idx_t));
        uint64_t made = 0;
        if (int rc = run_fmw_build<idx_t>(be, dB, n, primary, dSA, (uint32_t)s, hc.base, room, hc.base + off_ws, p, &made)) return rc;
        be.d2h(index, hc.base, made);
        be.sync();
        blob_mark_resident(hc, index, made);
        return CAPS_SA_OK;
    });
}

// count on device arrays; `hdr`: the header when the caller has read it already (the host forms), else it is read back here
inline int run_fm_count(Backend& be, const void* dIndex, uint64_t index_bytes, const uint64_t* hdr, const void* dPat, const void* dPatOff, uint64_t q,
                        void* dFirst, void* dCount)
{
    uint64_t h[FM_HDR_WORDS];
    if (hdr) std::memcpy(h, hdr, sizeof h);
    else { be.d2h(h, dIndex, sizeof h); be.sync(); }
    FmView v;
    FmwView w;
    if (int rc = fm_check_any(be, h, index_bytes, dIndex, v, w)) return rc;
    if (q == 0) return CAPS_SA_OK;
    uint64_t* words = call_words(be);
    uint32_t* flags = reinterpret_cast<uint32_t*>(words);
    const uint32_t g = capped_grid(std::min<uint64_t>((q + FM_NT - 1) / FM_NT, 1u << 20), FM_NT);
    be.memset(words, 0, sizeof(uint64_t));
    CAPS_LAUNCH(fm_check_kernel, g, FM_NT, be, static_cast<const uint64_t*>(dPatOff), q, (const uint64_t*)nullptr, (const uint64_t*)nullptr, v.n, flags);
    uint32_t f = 0;
    be.d2h(&f, flags, sizeof f);
    be.sync();
    if (f & 1u) return fail(CAPS_SA_EINVAL, "pattern offsets are not monotone");
    if (v.n == 0) {
        be.memset(dFirst, 0, q * sizeof(uint64_t));
        be.memset(dCount, 0, q * sizeof(uint64_t));
    } else if (w.Lv) {
        if (h[FMH_IDX_BYTES] == 4)
            CAPS_LAUNCH((fmw_count_q_kernel<uint32_t>), g, FM_NT, be, w, static_cast<const uint8_t*>(dPat), static_cast<const uint64_t*>(dPatOff), q,
                        static_cast<uint64_t*>(dFirst), static_cast<uint64_t*>(dCount));
        else
            CAPS_LAUNCH((fmw_count_q_kernel<uint64_t>), g, FM_NT, be, w, static_cast<const uint8_t*>(dPat), static_cast<const uint64_t*>(dPatOff), q,
                        static_cast<uint64_t*>(dFirst), static_cast<uint64_t*>(dCount));
    } else if (h[FMH_IDX_BYTES] == 4) {
        CAPS_LAUNCH((fm_count_kernel<uint32_t>), g, FM_NT, be, v, static_cast<const uint8_t*>(dPat), static_cast<const uint64_t*>(dPatOff), q,
                    static_cast<uint64_t*>(dFirst), static_cast<uint64_t*>(dCount));
    } else {
        CAPS_LAUNCH((fm_count_kernel<uint64_t>), g, FM_NT, be, v, static_cast<const uint8_t*>(dPat), static_cast<const uint64_t*>(dPatOff), q,
                    static_cast<uint64_t*>(dFirst), static_cast<uint64_t*>(dCount));
    }
    be.sync();
    return CAPS_SA_OK;
}

inline int fm_count_device(const void* dIndex, uint64_t index_bytes, const void* dPat, const void* dPatOff, uint64_t q, void* dFirst, void* dCount,
                           void* stream)
{
    if (!dIndex) return fail(CAPS_SA_EINVAL, "null index");
    if (index_bytes < FM_HDR_WORDS * sizeof(uint64_t)) return fail(CAPS_SA_EINVAL, "index_bytes is smaller than an FM-index header");
    if (q && (!dPatOff || !dFirst || !dCount)) return fail(CAPS_SA_EINVAL, "null pointer");
    return guarded([&]() -> int {
        Backend be(static_cast<decltype(Backend::stream)>(stream));
        return run_fm_count(be, dIndex, index_bytes, nullptr, dPat, dPatOff, q, dFirst, dCount);
    });
}

inline int run_fm_locate(Backend& be, const void* dIndex, uint64_t index_bytes, const uint64_t* hdr, const void* dFirst, const void* dCount,
                         const void* dOutOff, uint64_t q, void* dPos)
{
    uint64_t h[FM_HDR_WORDS];
    if (hdr) std::memcpy(h, hdr, sizeof h);
    else { be.d2h(h, dIndex, sizeof h); be.sync(); }
    FmView v;
    FmwView w;
    if (int rc = fm_check_any(be, h, index_bytes, dIndex, v, w)) return rc;
    if (v.s == 0 && v.n) return fail(CAPS_SA_EUNSUPPORTED, "this FM-index was built without SA samples: it can count, not locate");
    if (q == 0) return CAPS_SA_OK;
    uint64_t* words = call_words(be);
    uint32_t* flags = reinterpret_cast<uint32_t*>(words);
    const uint32_t g = capped_grid(std::min<uint64_t>((q + FM_NT - 1) / FM_NT, 1u << 20), FM_NT);
    be.memset(words, 0, sizeof(uint64_t));
    CAPS_LAUNCH(fm_check_kernel, g, FM_NT, be, static_cast<const uint64_t*>(dOutOff), q, static_cast<const uint64_t*>(dFirst),
                static_cast<const uint64_t*>(dCount), v.n, flags);
    uint32_t f = 0;
    uint64_t o_begin = 0, o_end = 0;
    be.d2h(&f, flags, sizeof f);
    be.d2h(&o_begin, dOutOff, sizeof(uint64_t));
    be.d2h(&o_end, static_cast<const uint64_t*>(dOutOff) + q, sizeof(uint64_t));
    be.sync();
    if (f & 1u) return fail(CAPS_SA_EINVAL, "output offsets are not monotone");
    if (f & 2u) return fail(CAPS_SA_EINVAL, "first + count > n");
    if (o_end == o_begin || v.n == 0) return CAPS_SA_OK;
    if (!dPos) return fail(CAPS_SA_EINVAL, "null pointer");
    const uint32_t lg = capped_grid(std::min<uint64_t>((o_end - o_begin + FM_NT - 1) / FM_NT, 1u << 20), FM_NT);
    if (w.Lv && h[FMH_IDX_BYTES] == 4)
        CAPS_LAUNCH((fmw_locate_kernel<uint32_t>), lg, FM_NT, be, w, static_cast<const uint64_t*>(dFirst), static_cast<const uint64_t*>(dCount),
                    static_cast<const uint64_t*>(dOutOff), q, o_begin, o_end, static_cast<uint64_t*>(dPos), flags);
    else if (w.Lv)
        CAPS_LAUNCH((fmw_locate_kernel<uint64_t>), lg, FM_NT, be, w, static_cast<const uint64_t*>(dFirst), static_cast<const uint64_t*>(dCount),
                    static_cast<const uint64_t*>(dOutOff), q, o_begin, o_end, static_cast<uint64_t*>(dPos), flags);
    else if (h[FMH_IDX_BYTES] == 4)
        CAPS_LAUNCH((fm_locate_kernel<uint32_t>), lg, FM_NT, be, v, static_cast<const uint64_t*>(dFirst), static_cast<const uint64_t*>(dCount),
                    static_cast<const uint64_t*>(dOutOff), q, o_begin, o_end, static_cast<uint64_t*>(dPos), flags);
    else
        CAPS_LAUNCH((fm_locate_kernel<uint64_t>), lg, FM_NT, be, v, static_cast<const uint64_t*>(dFirst), static_cast<const uint64_t*>(dCount),
                    static_cast<const uint64_t*>(dOutOff), q, o_begin, o_end, static_cast<uint64_t*>(dPos), flags);
    be.d2h(&f, flags, sizeof f);
    be.sync();
    if (f & 4u)
        return fail(CAPS_SA_EINVAL, "a locate walk did not reach a sampled row within sa_sample steps: the blob is not an index this library built");
    return CAPS_SA_OK;
}

inline int fm_locate_device(const void* dIndex, uint64_t index_bytes, const void* dFirst, const void* dCount, const void* dOutOff, uint64_t q,
                            void* dPos, void* stream)
{
    if (!dIndex) return fail(CAPS_SA_EINVAL, "null index");
    if (index_bytes < FM_HDR_WORDS * sizeof(uint64_t)) return fail(CAPS_SA_EINVAL, "index_bytes is smaller than an FM-index header");
    if (q && (!dOutOff || !dFirst || !dCount)) return fail(CAPS_SA_EINVAL, "null pointer");
    return guarded([&]() -> int {
        Backend be(static_cast<decltype(Backend::stream)>(stream));
        return run_fm_locate(be, dIndex, index_bytes, nullptr, dFirst, dCount, dOutOff, q, dPos);
    });
}

// the host forms: the blob at the head of the host-path block (uploaded unless it is the one there already), the query arrays behind it
inline void blob_upload(HostPathCache& hc, Backend& be, int device, const void* index, uint64_t blob, size_t total)
{
    const bool resident = hc.blob_host == index && hc.blob_bytes == blob && hc.device == device && hc.bytes >= total && hc.base &&
                          std::memcmp(hc.blob_hdr, index, sizeof hc.blob_hdr) == 0 && hc.blob_sum == blob_body_sum(index, blob);
    if (resident) return;
    hc.blob_host = nullptr;
    host_block(hc, be, device, total);
    be.h2d(hc.base, index, blob);
    be.sync();
    blob_mark_resident(hc, index, blob);
}
// w: a call that answers wide blobs passes it (w->Lv = 0 for a narrow blob); without it a wide blob is CAPS_SA_EUNSUPPORTED
inline int fm_host_header(const void* index, uint64_t index_bytes, uint64_t* h, FmView& v, FmwView* w = nullptr)
{
    if (!index) return fail(CAPS_SA_EINVAL, "null index");
    if (index_bytes < FM_HDR_WORDS * sizeof(uint64_t)) return fail(CAPS_SA_EINVAL, "index_bytes is smaller than an FM-index header");
    std::memcpy(h, index, FM_HDR_WORDS * sizeof(uint64_t));
    if (w) *w = FmwView{};
    if (h[FMH_MAGIC] == FMW_MAGIC) {
        if (!w) return fail(CAPS_SA_EUNSUPPORTED, FMW_NOT_BUILT);
        if (index_bytes < FM_HDR_WORDS * sizeof(uint64_t) + FMW_TAB_BYTES) return fail(CAPS_SA_EINVAL, "index_bytes is smaller than the FM-index (truncated blob)");
        FmwTable t;
        std::memcpy(t.w, static_cast<const char*>(index) + FM_HDR_WORDS * sizeof(uint64_t), FMW_TAB_BYTES);
        return fmw_check(h, t.w, index_bytes, index, v, *w);
    }
    return fm_check_header(h, index_bytes, index, v);
}

inline int fm_count_host(const void* index, uint64_t index_bytes, const uint8_t* pat, const uint64_t* patoff, uint64_t q, uint64_t* first,
                         uint64_t* count, int device)
{
    uint64_t h[FM_HDR_WORDS];
    FmView v;
    FmwView w;
    if (int rc = fm_host_header(index, index_bytes, h, v, &w)) return rc;
    if (q == 0) return CAPS_SA_OK;
    if (!patoff || !first || !count) return fail(CAPS_SA_EINVAL, "null pointer");
    for (uint64_t j = 0; j < q; ++j)
        if (patoff[j + 1] < patoff[j]) return fail(CAPS_SA_EINVAL, "pattern offsets are not monotone");
    const uint64_t pbytes = patoff[q];
    if (pbytes && !pat) return fail(CAPS_SA_EINVAL, "null pointer");
    DeviceScope restore_device_;
    if (int rc = set_device(device)) return rc;
    return guarded([&]() -> int {
        HostPathCache& hc = host_cache();
        std::lock_guard<std::mutex> lock(hc.mu);
        Backend be(nullptr);
        const uint64_t blob = fm_blob_bytes(h);
        const size_t off_pat = align_up(blob), off_off = off_pat + align_up(pbytes + 1), off_first = off_off + align_up((q + 1) * 8),
                     off_count = off_first + align_up(q * 8);
        blob_upload(hc, be, device, index, blob, off_count + align_up(q * 8));
        be.h2d(hc.base + off_pat, pat, pbytes);
        be.h2d(hc.base + off_off, patoff, (q + 1) * 8);
        if (int rc = run_fm_count(be, hc.base, blob, h, hc.base + off_pat, hc.base + off_off, q, hc.base + off_first, hc.base + off_count)) return rc;
        be.d2h(first, hc.base + off_first, q * 8);
        be.d2h(count, hc.base + off_count, q * 8);
        be.sync();
        return CAPS_SA_OK;
    });
}

inline int fm_locate_host(const void* index, uint64_t index_bytes, const uint64_t* first, const uint64_t* count, const uint64_t* outoff, uint64_t q,
                          uint64_t* pos, int device)
{
    uint64_t h[FM_HDR_WORDS];
    FmView v;
    FmwView w;
    if (int rc = fm_host_header(index, index_bytes, h, v, &w)) return rc;
    if (v.s == 0 && v.n) return fail(CAPS_SA_EUNSUPPORTED, "this FM-index was built without SA samples: it can count, not locate");
    if (q == 0) return CAPS_SA_OK;
    if (!outoff || !first || !count) return fail(CAPS_SA_EINVAL, "null pointer");
    for (uint64_t j = 0; j < q; ++j) {
        if (outoff[j + 1] < outoff[j]) return fail(CAPS_SA_EINVAL, "output offsets are not monotone");
        if (first[j] > v.n || count[j] > v.n - first[j]) return fail(CAPS_SA_EINVAL, "first + count > n");
    }
    const uint64_t o_end = outoff[q];
    if (o_end > outoff[0] && !pos) return fail(CAPS_SA_EINVAL, "null pointer");
    DeviceScope restore_device_;
    if (int rc = set_device(device)) return rc;
    return guarded([&]() -> int {
        HostPathCache& hc = host_cache();
        std::lock_guard<std::mutex> lock(hc.mu);
        Backend be(nullptr);
        const uint64_t blob = fm_blob_bytes(h);
        const size_t off_first = align_up(blob), off_count = off_first + align_up(q * 8), off_off = off_count + align_up(q * 8),
                     off_pos = off_off + align_up((q + 1) * 8);
        blob_upload(hc, be, device, index, blob, off_pos + align_up(o_end * 8 + 8));
        be.h2d(hc.base + off_first, first, q * 8);
        be.h2d(hc.base + off_count, count, q * 8);
        be.h2d(hc.base + off_off, outoff, (q + 1) * 8);
        be.memset(hc.base + off_pos, 0xFF, o_end * 8 + 8);   // (slots beyond a query's hits come back as UINT64_MAX)
        if (int rc = run_fm_locate(be, hc.base, blob, h, hc.base + off_first, hc.base + off_count, hc.base + off_off, q, hc.base + off_pos)) return rc;
        be.d2h(pos + outoff[0], hc.base + off_pos + outoff[0] * 8, (o_end - outoff[0]) * 8);
        be.sync();
        return CAPS_SA_OK;
    });
}

// ---- text-position samples and extract (include/caps_sa_hip.h "FM-index: extract"; kernels.h fm_rowof_kernel, fm_extract_kernel) ----
// in place at dIndex (capacity bytes): the blob with samples becomes version 2 at distance t; synchronises.  hdr: the header when the
// caller has read it already; hdr_out: the header as written.  Nothing is written before every refusal of the arguments.
inline int run_fm_add_text_samples(Backend& be, char* dIndex, uint64_t capacity, uint32_t t, const uint64_t* hdr, uint64_t* hdr_out)
{
    uint64_t h[FM_HDR_WORDS];
    if (hdr) std::memcpy(h, hdr, sizeof h);
    else { be.d2h(h, dIndex, sizeof h); be.sync(); }
    FmView v;
    if (h[FMH_MAGIC] == FMW_MAGIC) return fail(CAPS_SA_EUNSUPPORTED, FMW_NOT_BUILT);
    if (int rc = fm_check_header(h, capacity, dIndex, v)) return rc;
    if (v.s == 0) return fail(CAPS_SA_EUNSUPPORTED, "this FM-index was built without SA samples: text samples are taken from them");
    if (t < v.s) return fail(CAPS_SA_EINVAL, "text_sample must be a power of two in sa_sample .. 1024");
    const int W = (int)h[FMH_IDX_BYTES];
    const FmTextLayout tl = fm_text_layout(fm_layout(v.n, v.s, W), v.n, t, W);
    if (capacity < tl.total) return fail(CAPS_SA_EINVAL, "index_bytes too small (caps_sa_hip_fm_index_bytes_ex)");
    const bool was_text = h[FMH_VERSION] == FM_VERSION_TEXT;
    h[FMH_VERSION] = FM_VERSION;
    for (uint32_t k = FMH_T; k < FM_HDR_WORDS; ++k) h[k] = 0;
    uint32_t f = 0;
    if (tl.total > tl.off) be.memset(dIndex + tl.off, 0, tl.total - tl.off);
    if (v.n) {
        uint64_t* words = call_words(be);
        uint32_t* flags = reinterpret_cast<uint32_t*>(words);
        be.memset(words, 0, sizeof(uint64_t));
        const uint64_t mark_words = v.n_blocks * (W == 4 ? FmGeom<uint32_t>::MWN : FmGeom<uint64_t>::MWN);
        const uint32_t g = capped_grid(std::min<uint64_t>((mark_words + FM_NT - 1) / FM_NT, 1u << 20), FM_NT);
        const uint32_t cg = capped_grid(std::min<uint64_t>((tl.m + FM_NT - 1) / FM_NT, 1u << 20), FM_NT);
        if (W == 4) {
            uint32_t* rowof = reinterpret_cast<uint32_t*>(dIndex + tl.off);
            CAPS_LAUNCH((fm_rowof_kernel<uint32_t>), g, FM_NT, be, v, t, tl.m, rowof);
            CAPS_LAUNCH((fm_rowof_check_kernel<uint32_t>), cg, FM_NT, be, (const uint32_t*)rowof, tl.m, v.n, flags);
        } else {
            uint64_t* rowof = reinterpret_cast<uint64_t*>(dIndex + tl.off);
            CAPS_LAUNCH((fm_rowof_kernel<uint64_t>), g, FM_NT, be, v, t, tl.m, rowof);
            CAPS_LAUNCH((fm_rowof_check_kernel<uint64_t>), cg, FM_NT, be, (const uint64_t*)rowof, tl.m, v.n, flags);
        }
        be.d2h(&f, flags, sizeof f);
        be.sync();
    }
    if (!(f & 8u)) {
        h[FMH_VERSION] = FM_VERSION_TEXT;
        h[FMH_T] = t; h[FMH_NTEXT] = tl.m; h[FMH_OFF_ROWOF] = tl.off; h[FMH_TOTAL2] = tl.total;
    }
    if (!(f & 8u) || was_text) {                             // (refused: a version-1 header stays as it is, a version-2 one falls back to it)
        be.h2d(dIndex, h, sizeof h);
        be.sync();
    }
    if (hdr_out) std::memcpy(hdr_out, h, sizeof h);
    if (f & 8u)
        return fail(CAPS_SA_EINVAL, "the SA samples do not hold every multiple of text_sample once: the blob is not an index this library built");
    return CAPS_SA_OK;
}

inline int fm_add_text_samples_device(void* dIndex, uint64_t index_bytes, uint32_t t, void* stream)
{
    if (!dIndex) return fail(CAPS_SA_EINVAL, "null index");
    if (index_bytes < FM_HDR_WORDS * sizeof(uint64_t)) return fail(CAPS_SA_EINVAL, "index_bytes is smaller than an FM-index header");
    if (!fm_sample_ok(t)) return fail(CAPS_SA_EINVAL, "text_sample must be a power of two in sa_sample .. 1024");
    return guarded([&]() -> int {
        Backend be(static_cast<decltype(Backend::stream)>(stream));
        return run_fm_add_text_samples(be, static_cast<char*>(dIndex), index_bytes, t, nullptr, nullptr);
    });
}

// the host form: the version-1 part up (unless it is the blob there already), the section built behind it, header and section down.
// The device copy is then the caller's new blob and is marked so: the next host query does not upload it again.
inline int fm_add_text_samples_host(void* index, uint64_t index_bytes, uint32_t t, int device)
{
    uint64_t h[FM_HDR_WORDS];
    FmView v;
    if (!fm_sample_ok(t)) return fail(CAPS_SA_EINVAL, "text_sample must be a power of two in sa_sample .. 1024");
    if (int rc = fm_host_header(index, index_bytes, h, v)) return rc;
    if (v.s == 0) return fail(CAPS_SA_EUNSUPPORTED, "this FM-index was built without SA samples: text samples are taken from them");
    if (t < v.s) return fail(CAPS_SA_EINVAL, "text_sample must be a power of two in sa_sample .. 1024");
    const int W = (int)h[FMH_IDX_BYTES];
    const FmTextLayout tl = fm_text_layout(fm_layout(v.n, v.s, W), v.n, t, W);
    if (index_bytes < tl.total) return fail(CAPS_SA_EINVAL, "index_bytes too small (caps_sa_hip_fm_index_bytes_ex)");
    DeviceScope restore_device_;
    if (int rc = set_device(device)) return rc;
    return guarded([&]() -> int {
        HostPathCache& hc = host_cache();
        std::lock_guard<std::mutex> lock(hc.mu);
        Backend be(nullptr);
        const uint64_t room = std::max<uint64_t>(tl.total, fm_blob_bytes(h));    // (a version-2 blob at a smaller distance is the larger)
        blob_upload(hc, be, device, index, fm_blob_bytes(h), (size_t)room + WS_ALIGN);
        hc.blob_host = nullptr;                                // (the block is about to differ from the caller's blob)
        uint64_t out[FM_HDR_WORDS];
        std::memcpy(out, h, sizeof out);
        const int rc = run_fm_add_text_samples(be, hc.base, room, t, h, out);
        if (rc != CAPS_SA_OK && rc != CAPS_SA_EINVAL) return rc;
        const std::string msg = last_error_ref();
        std::memcpy(index, out, sizeof out);
        if (rc == CAPS_SA_OK) {
            if (tl.total > tl.off) be.d2h(static_cast<char*>(index) + tl.off, hc.base + tl.off, tl.total - tl.off);
            be.sync();
            blob_mark_resident(hc, index, tl.total);
        }
        last_error_ref() = msg;
        return rc;
    });
}

inline size_t fm_extract_plan_bytes(uint64_t q) { return align_up((q + 1) * sizeof(uint64_t)); }     // the workspace: pre u64[q + 1]
inline int fm_extract_workspace_bytes(uint64_t q, uint64_t* bytes)
{
    if (!bytes) return fail(CAPS_SA_EINVAL, "bad argument");
    if (q > (1ull << 56)) return fail(CAPS_SA_EINVAL, "too many queries");
    *bytes = ws_reported(fm_extract_plan_bytes(q));
    return CAPS_SA_OK;
}

// extract on device arrays; pre: u64[q + 1] of the workspace (256-byte aligned); `hdr` as in run_fm_count
inline int run_fm_extract(Backend& be, const void* dIndex, uint64_t index_bytes, const uint64_t* hdr, const void* dStart, const void* dOutOff,
                          uint64_t q, void* dText, uint64_t* pre)
{
    uint64_t h[FM_HDR_WORDS];
    if (hdr) std::memcpy(h, hdr, sizeof h);
    else { be.d2h(h, dIndex, sizeof h); be.sync(); }
    FmView v;
    if (h[FMH_MAGIC] == FMW_MAGIC) return fail(CAPS_SA_EUNSUPPORTED, FMW_NOT_BUILT);
    if (int rc = fm_check_header(h, index_bytes, dIndex, v)) return rc;
    if (h[FMH_VERSION] != FM_VERSION_TEXT)
        return fail(CAPS_SA_EUNSUPPORTED, "this FM-index has no text-position samples (format version 1): caps_sa_hip_fm_add_text_samples first");
    if (q == 0) return CAPS_SA_OK;
    uint64_t* words = call_words(be);
    uint32_t* flags = reinterpret_cast<uint32_t*>(words);
    const uint32_t sh = (uint32_t)__builtin_ctz(v.t);
    const uint32_t g = capped_grid(std::min<uint64_t>((q + FM_NT - 1) / FM_NT, 1u << 20), FM_NT);
    be.memset(words, 0, sizeof(uint64_t));
    CAPS_LAUNCH(fm_extract_plan_kernel, g, FM_NT, be, static_cast<const uint64_t*>(dStart), static_cast<const uint64_t*>(dOutOff), q, v.n, sh, pre, flags);
    CAPS_LAUNCH(fm_scan_kernel, 1, FM_NT, be, pre, q, 0u, 1u, pre + q);
    uint32_t f = 0;
    uint64_t lanes = 0;
    be.d2h(&f, flags, sizeof f);
    be.d2h(&lanes, pre + q, sizeof lanes);
    be.sync();
    if (f & 1u) return fail(CAPS_SA_EINVAL, "output offsets are not monotone");
    if (f & 2u) return fail(CAPS_SA_EINVAL, "start + length > n");
    if (lanes == 0) return CAPS_SA_OK;
    if (!dText) return fail(CAPS_SA_EINVAL, "null pointer");
    static const bool bytes_only = std::getenv("CAPS_SA_FM_EXTRACT_BYTES") != nullptr;      // (measurement: byte stores only)
    const uint32_t eg = capped_grid(std::min<uint64_t>((lanes + FM_NT - 1) / FM_NT, 1u << 20), FM_NT);
    const uint64_t* s = static_cast<const uint64_t*>(dStart);
    const uint64_t* o = static_cast<const uint64_t*>(dOutOff);
    uint8_t* text = static_cast<uint8_t*>(dText);
    if (h[FMH_IDX_BYTES] == 4) {
        if (bytes_only) CAPS_LAUNCH((fm_extract_kernel<uint32_t, false>), eg, FM_NT, be, v, s, o, (const uint64_t*)pre, q, lanes, text, flags);
        else CAPS_LAUNCH((fm_extract_kernel<uint32_t, true>), eg, FM_NT, be, v, s, o, (const uint64_t*)pre, q, lanes, text, flags);
    } else {
        if (bytes_only) CAPS_LAUNCH((fm_extract_kernel<uint64_t, false>), eg, FM_NT, be, v, s, o, (const uint64_t*)pre, q, lanes, text, flags);
        else CAPS_LAUNCH((fm_extract_kernel<uint64_t, true>), eg, FM_NT, be, v, s, o, (const uint64_t*)pre, q, lanes, text, flags);
    }
    be.d2h(&f, flags, sizeof f);
    be.sync();
    if (f & 4u)
        return fail(CAPS_SA_EINVAL, "an extract walk met the '$' row or row 0 below its text sample: the blob is not an index this library built");
    return CAPS_SA_OK;
}

inline int fm_extract_device(const void* dIndex, uint64_t index_bytes, const void* dStart, const void* dOutOff, uint64_t q, void* dText,
                             void* workspace, uint64_t workspace_bytes, void* stream)
{
    if (!dIndex) return fail(CAPS_SA_EINVAL, "null index");
    if (index_bytes < FM_HDR_WORDS * sizeof(uint64_t)) return fail(CAPS_SA_EINVAL, "index_bytes is smaller than an FM-index header");
    if (q && (!dStart || !dOutOff)) return fail(CAPS_SA_EINVAL, "null pointer");
    uint64_t need = 0;
    if (int rc = fm_extract_workspace_bytes(q, &need)) return rc;
    const size_t layout = fm_extract_plan_bytes(q);
    if (int rc = ws_check(workspace, workspace_bytes, layout, "workspace too small (caps_sa_hip_fm_extract_workspace_bytes)", WS_STRICT)) return rc;
    return guarded([&]() -> int {
        Backend be(static_cast<decltype(Backend::stream)>(stream));
        DevAllocs da(be);                                    // a null workspace: allocated here, freed on return
        uint64_t* pre = q ? reinterpret_cast<uint64_t*>(ws_carve(da, workspace, layout)) : nullptr;
        return run_fm_extract(be, dIndex, index_bytes, nullptr, dStart, dOutOff, q, dText, pre);
    });
}

inline int fm_extract_host(const void* index, uint64_t index_bytes, const uint64_t* start, const uint64_t* outoff, uint64_t q, uint8_t* text,
                           int device)
{
    uint64_t h[FM_HDR_WORDS];
    FmView v;
    if (int rc = fm_host_header(index, index_bytes, h, v)) return rc;
    if (h[FMH_VERSION] != FM_VERSION_TEXT)
        return fail(CAPS_SA_EUNSUPPORTED, "this FM-index has no text-position samples (format version 1): caps_sa_hip_fm_add_text_samples first");
    if (q == 0) return CAPS_SA_OK;
    if (!outoff || !start) return fail(CAPS_SA_EINVAL, "null pointer");
    for (uint64_t j = 0; j < q; ++j) {
        if (outoff[j + 1] < outoff[j]) return fail(CAPS_SA_EINVAL, "output offsets are not monotone");
        if (start[j] > v.n || outoff[j + 1] - outoff[j] > v.n - start[j]) return fail(CAPS_SA_EINVAL, "start + length > n");
    }
    const uint64_t o_begin = outoff[0], o_end = outoff[q];
    if (o_end > o_begin && !text) return fail(CAPS_SA_EINVAL, "null pointer");
    uint64_t ws = 0;
    if (int rc = fm_extract_workspace_bytes(q, &ws)) return rc;
    DeviceScope restore_device_;
    if (int rc = set_device(device)) return rc;
    return guarded([&]() -> int {
        HostPathCache& hc = host_cache();
        std::lock_guard<std::mutex> lock(hc.mu);
        Backend be(nullptr);
        const uint64_t blob = fm_blob_bytes(h);
        const size_t off_start = align_up(blob), off_off = off_start + align_up(q * 8), off_ws = off_off + align_up((q + 1) * 8), off_text = off_ws + align_up(ws);
        blob_upload(hc, be, device, index, blob, off_text + align_up(o_end + 8));
        be.h2d(hc.base + off_start, start, q * 8);
        be.h2d(hc.base + off_off, outoff, (q + 1) * 8);
        if (int rc = run_fm_extract(be, hc.base, blob, h, hc.base + off_start, hc.base + off_off, q, hc.base + off_text,
                                    reinterpret_cast<uint64_t*>(hc.base + off_ws)))
            return rc;
        if (o_end > o_begin) be.d2h(text + o_begin, hc.base + off_text + o_begin, o_end - o_begin);
        be.sync();
        return CAPS_SA_OK;
    });
}

// ---- matching statistics and MEMs (include/caps_sa_hip.h "FM-index: matching statistics"; kernels.h fm_match_kernel, fm_mem_*) ----
constexpr uint64_t FM_MAX_PATTERN = 0xFFFFFFFFull;           // bytes of a pattern: len[], a MEM's start and length are 32-bit
constexpr uint64_t FM_MEM_BYTES = 32;

// the entry checks of both calls on the caller's device offsets: monotone, no pattern above FM_MAX_PATTERN; -> [o_begin, o_end)
inline int fm_match_offsets(Backend& be, const void* dPatOff, uint64_t q, uint64_t n, uint64_t& o_begin, uint64_t& o_end)
{
    uint64_t* words = call_words(be);
    uint32_t* flags = reinterpret_cast<uint32_t*>(words);
    const uint32_t g = capped_grid(std::min<uint64_t>((q + FM_NT - 1) / FM_NT, 1u << 20), FM_NT);
    be.memset(words, 0, sizeof(uint64_t));
    CAPS_LAUNCH(fm_check_kernel, g, FM_NT, be, static_cast<const uint64_t*>(dPatOff), q, (const uint64_t*)nullptr, (const uint64_t*)nullptr, n, flags);
    CAPS_LAUNCH(fm_patlen_check_kernel, g, FM_NT, be, static_cast<const uint64_t*>(dPatOff), q, FM_MAX_PATTERN, flags);
    uint32_t f = 0;
    be.d2h(&f, flags, sizeof f);
    be.d2h(&o_begin, dPatOff, sizeof(uint64_t));
    be.d2h(&o_end, static_cast<const uint64_t*>(dPatOff) + q, sizeof(uint64_t));
    be.sync();
    if (f & 1u) return fail(CAPS_SA_EINVAL, "pattern offsets are not monotone");
    if (f & 16u) return fail(CAPS_SA_EINVAL, "a pattern is longer than 2^32 - 1 bytes");
    return CAPS_SA_OK;
}

// the match kernel over [o_begin, o_end) (not empty); n = 0: every length 0
inline void launch_fm_match(Backend& be, const FmView& v, const FmwView& w, int W, const void* dPat, const void* dPatOff, uint64_t q, uint64_t o_begin, uint64_t o_end,
                            uint32_t max_len, uint32_t* len, uint64_t* first, uint64_t* count)
{
    const uint64_t total = o_end - o_begin;
    if (v.n == 0) {
        be.memset(len, 0, total * sizeof(uint32_t));
        if (first) be.memset(first, 0, total * sizeof(uint64_t));
        if (count) be.memset(count, 0, total * sizeof(uint64_t));
        return;
    }
    const uint32_t g = capped_grid(std::min<uint64_t>((total + FM_NT - 1) / FM_NT, 1u << 20), FM_NT);
    if (w.Lv && W == 4)
        CAPS_LAUNCH((fmw_match_kernel<uint32_t>), g, FM_NT, be, w, static_cast<const uint8_t*>(dPat), static_cast<const uint64_t*>(dPatOff), q, o_begin,
                    o_end, max_len, len, first, count);
    else if (w.Lv)
        CAPS_LAUNCH((fmw_match_kernel<uint64_t>), g, FM_NT, be, w, static_cast<const uint8_t*>(dPat), static_cast<const uint64_t*>(dPatOff), q, o_begin,
                    o_end, max_len, len, first, count);
    else if (W == 4)
        CAPS_LAUNCH((fm_match_kernel<uint32_t>), g, FM_NT, be, v, static_cast<const uint8_t*>(dPat), static_cast<const uint64_t*>(dPatOff), q, o_begin,
                    o_end, max_len, len, first, count);
    else
        CAPS_LAUNCH((fm_match_kernel<uint64_t>), g, FM_NT, be, v, static_cast<const uint8_t*>(dPat), static_cast<const uint64_t*>(dPatOff), q, o_begin,
                    o_end, max_len, len, first, count);
}

// matching statistics on device arrays; `hdr` as in run_fm_count
inline int run_fm_match(Backend& be, const void* dIndex, uint64_t index_bytes, const uint64_t* hdr, const void* dPat, const void* dPatOff, uint64_t q,
                        uint32_t max_len, void* dLen, void* dFirst, void* dCount)
{
    uint64_t h[FM_HDR_WORDS];
    if (hdr) std::memcpy(h, hdr, sizeof h);
    else { be.d2h(h, dIndex, sizeof h); be.sync(); }
    FmView v;
    FmwView w;
    if (int rc = fm_check_any(be, h, index_bytes, dIndex, v, w)) return rc;
    if (q == 0) return CAPS_SA_OK;
    uint64_t o_begin = 0, o_end = 0;
    if (int rc = fm_match_offsets(be, dPatOff, q, v.n, o_begin, o_end)) return rc;
    if (o_end == o_begin) return CAPS_SA_OK;
    if (!dPat || !dLen) return fail(CAPS_SA_EINVAL, "null pointer");
    launch_fm_match(be, v, w, (int)h[FMH_IDX_BYTES], dPat, dPatOff, q, o_begin, o_end, max_len, static_cast<uint32_t*>(dLen),
                    static_cast<uint64_t*>(dFirst), static_cast<uint64_t*>(dCount));
    be.sync();
    return CAPS_SA_OK;
}

inline int fm_match_device(const void* dIndex, uint64_t index_bytes, const void* dPat, const void* dPatOff, uint64_t q, uint32_t max_len,
                           void* dLen, void* dFirst, void* dCount, void* stream)
{
    if (!dIndex) return fail(CAPS_SA_EINVAL, "null index");
    if (index_bytes < FM_HDR_WORDS * sizeof(uint64_t)) return fail(CAPS_SA_EINVAL, "index_bytes is smaller than an FM-index header");
    if (q && (!dPatOff || !dLen)) return fail(CAPS_SA_EINVAL, "null pointer");
    return guarded([&]() -> int {
        Backend be(static_cast<decltype(Backend::stream)>(stream));
        return run_fm_match(be, dIndex, index_bytes, nullptr, dPat, dPatOff, q, max_len, dLen, dFirst, dCount);
    });
}

// the host checks of the pattern arrays of both calls
inline int fm_match_host_check(const uint8_t* pat, const uint64_t* patoff, uint64_t q)
{
    if (!patoff) return fail(CAPS_SA_EINVAL, "null pointer");
    for (uint64_t j = 0; j < q; ++j) {
        if (patoff[j + 1] < patoff[j]) return fail(CAPS_SA_EINVAL, "pattern offsets are not monotone");
        if (patoff[j + 1] - patoff[j] > FM_MAX_PATTERN) return fail(CAPS_SA_EINVAL, "a pattern is longer than 2^32 - 1 bytes");
    }
    if (patoff[q] && !pat) return fail(CAPS_SA_EINVAL, "null pointer");
    return CAPS_SA_OK;
}

inline int fm_match_host(const void* index, uint64_t index_bytes, const uint8_t* pat, const uint64_t* patoff, uint64_t q, uint32_t max_len,
                         uint32_t* len, uint64_t* first, uint64_t* count, int device)
{
    uint64_t h[FM_HDR_WORDS];
    FmView v;
    FmwView w;
    if (int rc = fm_host_header(index, index_bytes, h, v, &w)) return rc;
    if (q == 0) return CAPS_SA_OK;
    if (!len) return fail(CAPS_SA_EINVAL, "null pointer");
    if (int rc = fm_match_host_check(pat, patoff, q)) return rc;
    const uint64_t pbytes = patoff[q], total = patoff[q] - patoff[0];
    if (total == 0) return CAPS_SA_OK;
    DeviceScope restore_device_;
    if (int rc = set_device(device)) return rc;
    return guarded([&]() -> int {
        HostPathCache& hc = host_cache();
        std::lock_guard<std::mutex> lock(hc.mu);
        Backend be(nullptr);
        const uint64_t blob = fm_blob_bytes(h);
        const size_t off_pat = align_up(blob), off_off = off_pat + align_up(pbytes + 1), off_len = off_off + align_up((q + 1) * 8),
                     off_first = off_len + align_up(total * 4), off_count = off_first + align_up(first ? total * 8 : 0);
        blob_upload(hc, be, device, index, blob, off_count + align_up(count ? total * 8 : 0));
        be.h2d(hc.base + off_pat, pat, pbytes);
        be.h2d(hc.base + off_off, patoff, (q + 1) * 8);
        if (int rc = run_fm_match(be, hc.base, blob, h, hc.base + off_pat, hc.base + off_off, q, max_len, hc.base + off_len,
                                  first ? hc.base + off_first : nullptr, count ? hc.base + off_count : nullptr))
            return rc;
        be.d2h(len, hc.base + off_len, total * 4);
        if (first) be.d2h(first, hc.base + off_first, total * 8);
        if (count) be.d2h(count, hc.base + off_count, total * 8);
        be.sync();
        return CAPS_SA_OK;
    });
}

// workspace of the MEM calls: len u32[total + 1] | first, count u64[total] each | flags -> slots u64[padded] | the columns' totals ->
// bases u64[cols], 256-byte aligned each.  The total + 1 flags are scanned as `cols` columns of `per` slots, one workgroup each.
constexpr uint64_t FM_MEM_COLS = 1024, FM_MEM_COL_MIN = 1u << 16;
struct FmMemPlan { size_t off_len, off_first, off_count, off_slot, off_base, bytes; uint64_t cols, per, padded; };
inline FmMemPlan fm_mem_plan(uint64_t total)
{
    FmMemPlan p;
    p.cols = std::min<uint64_t>(FM_MEM_COLS, (total + 1 + FM_MEM_COL_MIN - 1) / FM_MEM_COL_MIN);
    p.per = (total + 1 + p.cols - 1) / p.cols;
    p.padded = p.cols * p.per;
    p.off_len = 0;
    p.off_first = p.off_len + align_up((total + 1) * 4);
    p.off_count = p.off_first + align_up(total * 8);
    p.off_slot = p.off_count + align_up(total * 8);
    p.off_base = p.off_slot + align_up(p.padded * 8);
    p.bytes = p.off_base + align_up(FM_MEM_COLS * 8);
    return p;
}
inline int fm_mems_workspace_bytes(uint64_t total, uint64_t q, uint64_t* bytes)
{
    if (!bytes) return fail(CAPS_SA_EINVAL, "bad argument");
    if (total > (1ull << 56) || q > (1ull << 56)) return fail(CAPS_SA_EINVAL, "too many pattern bytes or patterns");
    *bytes = ws_reported(fm_mem_plan(total).bytes);
    return CAPS_SA_OK;
}

// MEMs on device arrays.  dMemOff is written whenever the header and the offsets pass (offsets_written); workspace: the caller's (at
// any alignment), or null: allocated here once the pattern bytes are known.  `hdr` as in run_fm_count.
inline int run_fm_mems(Backend& be, DevAllocs& da, const void* dIndex, uint64_t index_bytes, const uint64_t* hdr, const void* dPat, const void* dPatOff,
                       uint64_t q, uint32_t min_len, void* dMemOff, void* dMems, uint64_t mem_capacity, void* workspace, uint64_t workspace_bytes,
                       bool* offsets_written)
{
    if (offsets_written) *offsets_written = false;
    uint64_t h[FM_HDR_WORDS];
    if (hdr) std::memcpy(h, hdr, sizeof h);
    else { be.d2h(h, dIndex, sizeof h); be.sync(); }
    FmView v;
    FmwView w;
    if (int rc = fm_check_any(be, h, index_bytes, dIndex, v, w)) return rc;
    if (q == 0) {
        if (dMemOff) { be.memset(dMemOff, 0, sizeof(uint64_t)); be.sync(); }
        if (offsets_written) *offsets_written = dMemOff != nullptr;
        return CAPS_SA_OK;
    }
    uint64_t o_begin = 0, o_end = 0;
    if (int rc = fm_match_offsets(be, dPatOff, q, v.n, o_begin, o_end)) return rc;
    const uint64_t total = o_end - o_begin;
    if (total == 0 || v.n == 0) {
        be.memset(dMemOff, 0, (q + 1) * sizeof(uint64_t));
        be.sync();
        if (offsets_written) *offsets_written = true;
        return CAPS_SA_OK;
    }
    if (!dPat) return fail(CAPS_SA_EINVAL, "null pointer");
    const FmMemPlan p = fm_mem_plan(total);
    if (int rc = ws_check(workspace, workspace_bytes, p.bytes, "workspace too small (caps_sa_hip_fm_mems_workspace_bytes)")) return rc;
    char* ws = ws_carve(da, workspace, p.bytes);
    uint32_t* len = reinterpret_cast<uint32_t*>(ws + p.off_len);
    uint64_t* first = reinterpret_cast<uint64_t*>(ws + p.off_first);
    uint64_t* count = reinterpret_cast<uint64_t*>(ws + p.off_count);
    uint64_t* slot = reinterpret_cast<uint64_t*>(ws + p.off_slot);
    uint64_t* colbase = reinterpret_cast<uint64_t*>(ws + p.off_base);
    uint64_t* words = call_words(be);
    const uint64_t* off = static_cast<const uint64_t*>(dPatOff);
    launch_fm_match(be, v, w, (int)h[FMH_IDX_BYTES], dPat, dPatOff, q, o_begin, o_end, 0u, len, dMems ? first : nullptr, dMems ? count : nullptr);
    const uint32_t g = capped_grid(std::min<uint64_t>((p.padded + FM_NT - 1) / FM_NT, 1u << 20), FM_NT);
    const uint32_t qg = capped_grid(std::min<uint64_t>((q + 1 + FM_NT - 1) / FM_NT, 1u << 20), FM_NT);
    CAPS_LAUNCH(fm_mem_flag_kernel, g, FM_NT, be, (const uint32_t*)len, off, q, total, p.padded, std::max<uint32_t>(min_len, 1u), slot);
    CAPS_LAUNCH(fm_scan_kernel, (uint32_t)p.cols, FM_NT, be, slot, p.per, 0u, (uint32_t)p.cols, colbase);
    CAPS_LAUNCH(fm_scan_kernel, 1, FM_NT, be, colbase, p.cols, 0u, 1u, words + 1);
    CAPS_LAUNCH(fm_mem_off_kernel, qg, FM_NT, be, (const uint64_t*)slot, (const uint64_t*)colbase, p.per, off, q, total, static_cast<uint64_t*>(dMemOff));
    uint64_t found = 0;
    be.d2h(&found, words + 1, sizeof found);
    be.sync();
    if (offsets_written) *offsets_written = true;
    if (!dMems) return CAPS_SA_OK;
    if (found > mem_capacity) return fail(CAPS_SA_EINVAL, "mem_capacity is smaller than the number of MEMs (dMemOff[q]; a call with dMems = NULL counts them)");
    if (found) {
        CAPS_LAUNCH(fm_mem_write_kernel, g, FM_NT, be, (const uint32_t*)len, (const uint64_t*)first, (const uint64_t*)count, (const uint64_t*)slot,
                    (const uint64_t*)colbase, p.per, off, q, total, mem_capacity, static_cast<uint64_t*>(dMems));
        be.sync();
    }
    return CAPS_SA_OK;
}

inline int fm_mems_device(const void* dIndex, uint64_t index_bytes, const void* dPat, const void* dPatOff, uint64_t q, uint32_t min_len,
                          void* dMemOff, void* dMems, uint64_t mem_capacity, void* workspace, uint64_t workspace_bytes, void* stream)
{
    if (!dIndex) return fail(CAPS_SA_EINVAL, "null index");
    if (index_bytes < FM_HDR_WORDS * sizeof(uint64_t)) return fail(CAPS_SA_EINVAL, "index_bytes is smaller than an FM-index header");
    if (!dMemOff || (q && !dPatOff)) return fail(CAPS_SA_EINVAL, "null pointer");
    if (reinterpret_cast<uintptr_t>(dMems) & 7u) return fail(CAPS_SA_EINVAL, "dMems must be 8-byte aligned");
    return guarded([&]() -> int {
        Backend be(static_cast<decltype(Backend::stream)>(stream));
        DevAllocs da(be);                                    // a null workspace: allocated here, freed on return
        return run_fm_mems(be, da, dIndex, index_bytes, nullptr, dPat, dPatOff, q, min_len, dMemOff, dMems, mem_capacity, workspace, workspace_bytes,
                           nullptr);
    });
}

inline int fm_mems_host(const void* index, uint64_t index_bytes, const uint8_t* pat, const uint64_t* patoff, uint64_t q, uint32_t min_len,
                        uint64_t* memoff, void* mems, uint64_t mem_capacity, int device)
{
    uint64_t h[FM_HDR_WORDS];
    FmView v;
    FmwView w;
    if (int rc = fm_host_header(index, index_bytes, h, v, &w)) return rc;
    if (!memoff) return fail(CAPS_SA_EINVAL, "null pointer");
    if (q == 0) { memoff[0] = 0; return CAPS_SA_OK; }
    if (int rc = fm_match_host_check(pat, patoff, q)) return rc;
    const uint64_t pbytes = patoff[q], total = patoff[q] - patoff[0];
    if (total == 0 || v.n == 0) { std::memset(memoff, 0, (q + 1) * 8); return CAPS_SA_OK; }
    DeviceScope restore_device_;
    if (int rc = set_device(device)) return rc;
    return guarded([&]() -> int {
        HostPathCache& hc = host_cache();
        std::lock_guard<std::mutex> lock(hc.mu);
        Backend be(nullptr);
        DevAllocs da(be);
        const uint64_t blob = fm_blob_bytes(h), room = mems ? std::min(mem_capacity, total) : 0;
        const FmMemPlan p = fm_mem_plan(total);
        const size_t off_pat = align_up(blob), off_off = off_pat + align_up(pbytes + 1), off_memoff = off_off + align_up((q + 1) * 8),
                     off_ws = off_memoff + align_up((q + 1) * 8), off_mems = off_ws + ws_reported(p.bytes);   // (run_fm_mems aligns the workspace)
        blob_upload(hc, be, device, index, blob, off_mems + align_up(room * FM_MEM_BYTES + 8));
        be.h2d(hc.base + off_pat, pat, pbytes);
        be.h2d(hc.base + off_off, patoff, (q + 1) * 8);
        bool written = false;
        const int rc = run_fm_mems(be, da, hc.base, blob, h, hc.base + off_pat, hc.base + off_off, q, min_len, hc.base + off_memoff,
                                   mems ? hc.base + off_mems : nullptr, mem_capacity, hc.base + off_ws, ws_reported(p.bytes), &written);
        if (written) {
            be.d2h(memoff, hc.base + off_memoff, (q + 1) * 8);
            be.sync();
        }
        if (rc) return rc;
        if (mems && memoff[q]) be.d2h(mems, hc.base + off_mems, memoff[q] * FM_MEM_BYTES);
        be.sync();
        return CAPS_SA_OK;
    });
}

// ---- k-mers from SA and LCP (include/caps_sa_hip.h "k-mers from SA and LCP"; kernels.h kmer_*) --------------------------------------
// Workspace: next[n_tiles + 1] | cnt[n_tiles] | totals[2 * KMER_KEYS] | per-workgroup histogram columns[2 * KMER_KEYS][grid], 64-bit words.
struct KmerPlan {
    uint64_t n_tiles = 0;
    uint32_t grid = 1;                         // workgroups of the histogram kernels (= the length of a column)
    size_t off_next = 0, off_cnt = 0, off_tot = 0, off_hist = 0, bytes = 0;
};
inline KmerPlan kmer_plan(uint64_t n)
{
    KmerPlan p;
    p.n_tiles = (n + KMER_TILE - 1) / KMER_TILE;
    // a workgroup's LDS bins are 32 bits wide: at most 2^16 tiles (2^30 ranks) each
    p.grid = capped_grid(std::max<uint64_t>(std::min<uint64_t>(p.n_tiles, 1024), (p.n_tiles + 65535) / 65536), FM_NT);
    p.off_next = 0;
    p.off_cnt = p.off_next + align_up((p.n_tiles + 1) * 8);
    p.off_tot = p.off_cnt + align_up((p.n_tiles + 1) * 8);
    p.off_hist = p.off_tot + align_up(2 * KMER_KEYS * 8);
    p.bytes = p.off_hist + align_up((size_t)2 * KMER_KEYS * p.grid * 8);
    return p;
}
inline int kmer_workspace_bytes(uint64_t n, int idx_bytes, uint64_t* bytes)
{
    if (int rc = check_size_query(n, idx_bytes, bytes)) return rc;
    *bytes = ws_reported(kmer_plan(n).bytes);
    return CAPS_SA_OK;
}

// the workspace of one call: the caller's (aligned up, checked by kmer_check_ws before) or one of the call's own
struct KmerWs {
    char* base = nullptr;
    KmerPlan p;
    uint64_t* next() const { return reinterpret_cast<uint64_t*>(base + p.off_next); }
    uint64_t* cnt() const { return reinterpret_cast<uint64_t*>(base + p.off_cnt); }
    uint64_t* tot() const { return reinterpret_cast<uint64_t*>(base + p.off_tot); }
    uint64_t* hist() const { return reinterpret_cast<uint64_t*>(base + p.off_hist); }
};
inline int kmer_check_ws(void* workspace, uint64_t workspace_bytes, uint64_t n)
{
    return ws_check(workspace, workspace_bytes, kmer_plan(n).bytes, "workspace too small (caps_sa_hip_kmer_workspace_bytes)");
}
inline KmerWs kmer_ws(DevAllocs& da, void* workspace, uint64_t n)
{
    KmerWs w;
    w.p = kmer_plan(n);
    w.base = ws_carve(da, workspace, w.p.bytes);
    return w;
}
inline int kmer_check_counts(uint64_t k, uint64_t min_count, uint64_t max_count)
{
    if (k == 0) return fail(CAPS_SA_EINVAL, "k must be at least 1");
    if (max_count && min_count > max_count) return fail(CAPS_SA_EINVAL, "min_count > max_count");
    return CAPS_SA_OK;
}

// next[t] = the first head at or after tile t (1 <= k <= n, n >= 1)
template <typename idx_t>
void run_kmer_heads(Backend& be, const idx_t* dLCP, uint64_t n, uint64_t k, const KmerWs& w)
{
    const uint32_t tg = capped_grid(std::min<uint64_t>(w.p.n_tiles, 1u << 20), FM_NT);
    CAPS_LAUNCH((kmer_head_kernel<idx_t>), tg, FM_NT, be, dLCP, n, k, w.p.n_tiles, w.next());
    CAPS_LAUNCH(kmer_next_kernel, 1, FM_NT, be, w.next(), w.p.n_tiles, n);
}

// the table: counts, and with dRec the records; *found is written whenever the call gets as far as counting
template <typename idx_t>
int run_kmers(Backend& be, const idx_t* dSA, const idx_t* dLCP, uint64_t n, uint64_t k, uint64_t min_count, uint64_t max_count, void* dRec,
              uint64_t capacity, uint64_t* found, const KmerWs& w)
{
    *found = 0;
    if (n == 0 || k > n) return CAPS_SA_OK;
    if (min_count == 0) min_count = 1;
    run_kmer_heads<idx_t>(be, dLCP, n, k, w);
    const uint32_t tg = capped_grid(std::min<uint64_t>(w.p.n_tiles, 1u << 20), FM_NT);
    CAPS_LAUNCH((kmer_run_kernel<idx_t, KMER_COUNT>), tg, FM_NT, be, dSA, dLCP, n, k, w.p.n_tiles, (const uint64_t*)w.next(), min_count, max_count,
                w.cnt(), (uint64_t*)nullptr, (uint64_t)0, 0u, (uint64_t*)nullptr);
    CAPS_LAUNCH(fm_scan_kernel, 1, FM_NT, be, w.cnt(), w.p.n_tiles, 0u, 1u, w.tot());
    be.d2h(found, w.tot(), sizeof(uint64_t));
    be.sync();
    if (!dRec) return CAPS_SA_OK;
    if (*found > capacity) return fail(CAPS_SA_EINVAL, "capacity is smaller than the number of k-mers (*n_records; a call with dRecords = NULL counts them)");
    if (*found) {
        CAPS_LAUNCH((kmer_run_kernel<idx_t, KMER_WRITE>), tg, FM_NT, be, dSA, dLCP, n, k, w.p.n_tiles, (const uint64_t*)w.next(), min_count, max_count,
                    w.cnt(), static_cast<uint64_t*>(dRec), capacity, 0u, (uint64_t*)nullptr);
        be.sync();
    }
    return CAPS_SA_OK;
}

template <typename idx_t>
int run_kmer_spectrum(Backend& be, const idx_t* dSA, const idx_t* dLCP, uint64_t n, uint64_t k, uint32_t bins, uint64_t* hist, const KmerWs& w)
{
    std::memset(hist, 0, ((size_t)bins + 1) * sizeof(uint64_t));
    if (n == 0 || k > n) return CAPS_SA_OK;
    run_kmer_heads<idx_t>(be, dLCP, n, k, w);
    CAPS_LAUNCH((kmer_run_kernel<idx_t, KMER_SPECTRUM>), w.p.grid, FM_NT, be, dSA, dLCP, n, k, w.p.n_tiles, (const uint64_t*)w.next(), (uint64_t)1,
                (uint64_t)0, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, bins, w.hist());
    CAPS_LAUNCH(fm_scan_kernel, bins + 1, FM_NT, be, w.hist(), (uint64_t)w.p.grid, 0u, bins + 1, w.tot());
    be.d2h(hist, w.tot(), ((size_t)bins + 1) * sizeof(uint64_t));
    be.sync();
    return CAPS_SA_OK;
}

template <typename idx_t>
int run_kmer_census(Backend& be, const idx_t* dSA, const idx_t* dLCP, uint64_t n, uint32_t max_k, uint64_t* distinct, uint64_t* unique, const KmerWs& w)
{
    std::memset(distinct, 0, ((size_t)max_k + 1) * sizeof(uint64_t));
    std::memset(unique, 0, ((size_t)max_k + 1) * sizeof(uint64_t));
    if (n == 0) return CAPS_SA_OK;
    CAPS_LAUNCH((kmer_census_kernel<idx_t>), w.p.grid, FM_NT, be, dSA, dLCP, n, max_k, w.p.n_tiles, w.hist());
    CAPS_LAUNCH(fm_scan_kernel, max_k + 1, FM_NT, be, w.hist(), (uint64_t)w.p.grid, 0u, max_k + 1, w.tot());
    CAPS_LAUNCH(fm_scan_kernel, max_k + 1, FM_NT, be, w.hist(), (uint64_t)w.p.grid, KMER_KEYS, max_k + 1, w.tot());
    std::vector<uint64_t> t(2 * KMER_KEYS);
    be.d2h(t.data(), w.tot(), t.size() * sizeof(uint64_t));
    be.sync();
    int64_t d = 0, u = 0;                                   // the differences summed from the left
    for (uint32_t k = 1; k <= max_k; ++k) {
        d += (int64_t)t[k];
        u += (int64_t)t[KMER_KEYS + k];
        distinct[k] = (uint64_t)d;
        unique[k] = (uint64_t)u;
    }
    return CAPS_SA_OK;
}

template <typename idx_t>
int kmers_device(const void* dSA, const void* dLCP, uint64_t n, uint64_t k, uint64_t min_count, uint64_t max_count, void* dRec, uint64_t capacity,
                 uint64_t* n_records, void* workspace, uint64_t workspace_bytes, void* stream)
{
    if (int rc = check_arrays<idx_t>(n, !dSA || !dLCP, "null pointer")) return rc;
    if (!n_records) return fail(CAPS_SA_EINVAL, "null pointer");
    if (int rc = kmer_check_counts(k, min_count, max_count)) return rc;
    if (reinterpret_cast<uintptr_t>(dRec) & 7u) return fail(CAPS_SA_EINVAL, "dRecords must be 8-byte aligned");
    if (int rc = kmer_check_ws(workspace, workspace_bytes, n)) return rc;
    return guarded([&]() -> int {
        Backend be(static_cast<decltype(Backend::stream)>(stream));
        DevAllocs da(be);
        KmerWs w;
        if (n && k <= n) w = kmer_ws(da, workspace, n);
        return run_kmers<idx_t>(be, static_cast<const idx_t*>(dSA), static_cast<const idx_t*>(dLCP), n, k, min_count, max_count, dRec, capacity,
                                n_records, w);
    });
}
template <typename idx_t>
int kmer_spectrum_device(const void* dSA, const void* dLCP, uint64_t n, uint64_t k, uint32_t bins, uint64_t* hist, void* workspace,
                         uint64_t workspace_bytes, void* stream)
{
    if (int rc = check_arrays<idx_t>(n, !dSA || !dLCP, "null pointer")) return rc;
    if (!hist) return fail(CAPS_SA_EINVAL, "null pointer");
    if (k == 0) return fail(CAPS_SA_EINVAL, "k must be at least 1");
    if (bins < 1 || bins > KMER_MAX_BINS) return fail(CAPS_SA_EINVAL, "bins must be in 1 .. 1024");
    if (int rc = kmer_check_ws(workspace, workspace_bytes, n)) return rc;
    return guarded([&]() -> int {
        Backend be(static_cast<decltype(Backend::stream)>(stream));
        DevAllocs da(be);
        KmerWs w;
        if (n && k <= n) w = kmer_ws(da, workspace, n);
        return run_kmer_spectrum<idx_t>(be, static_cast<const idx_t*>(dSA), static_cast<const idx_t*>(dLCP), n, k, bins, hist, w);
    });
}
template <typename idx_t>
int kmer_census_device(const void* dSA, const void* dLCP, uint64_t n, uint32_t max_k, uint64_t* distinct, uint64_t* unique, void* workspace,
                       uint64_t workspace_bytes, void* stream)
{
    if (int rc = check_arrays<idx_t>(n, !dSA || !dLCP, "null pointer")) return rc;
    if (!distinct || !unique) return fail(CAPS_SA_EINVAL, "null pointer");
    if (max_k < 1 || max_k > KMER_MAX_BINS) return fail(CAPS_SA_EINVAL, "max_k must be in 1 .. 1024");
    if (int rc = kmer_check_ws(workspace, workspace_bytes, n)) return rc;
    return guarded([&]() -> int {
        Backend be(static_cast<decltype(Backend::stream)>(stream));
        DevAllocs da(be);
        KmerWs w;
        if (n) w = kmer_ws(da, workspace, n);
        return run_kmer_census<idx_t>(be, static_cast<const idx_t*>(dSA), static_cast<const idx_t*>(dLCP), n, max_k, distinct, unique, w);
    });
}

// host SA / LCP: both up into buffers of the call's own (UploadedSaLcp), the device form on them, the records down
template <typename idx_t>
int kmers_host(const idx_t* SA, const idx_t* LCP, uint64_t n, uint64_t k, uint64_t min_count, uint64_t max_count, void* records, uint64_t capacity,
               uint64_t* n_records, int device)
{
    if (int rc = check_arrays<idx_t>(n, !SA || !LCP, "null pointer")) return rc;
    if (!n_records) return fail(CAPS_SA_EINVAL, "null pointer");
    if (int rc = kmer_check_counts(k, min_count, max_count)) return rc;
    if (reinterpret_cast<uintptr_t>(records) & 7u) return fail(CAPS_SA_EINVAL, "records must be 8-byte aligned");
    if (n == 0 || k > n) { *n_records = 0; return CAPS_SA_OK; }
    DeviceScope restore_device_;
    if (int rc = set_device(device)) return rc;
    return guarded([&]() -> int {
        Backend be(nullptr);
        DevAllocs da(be);
        UploadedSaLcp<idx_t> a(be, da, SA, LCP, n);
        const KmerWs w = kmer_ws(da, nullptr, n);
        if (int rc = run_kmers<idx_t>(be, a.sa, a.lcp, n, k, min_count, max_count, nullptr, 0, n_records, w)) return rc;
        if (!records) return CAPS_SA_OK;
        if (*n_records > capacity) return fail(CAPS_SA_EINVAL, "capacity is smaller than the number of k-mers (*n_records; a call with records = NULL counts them)");
        if (*n_records == 0) return CAPS_SA_OK;
        const uint64_t found = *n_records;
        uint64_t* dRec = da.get<uint64_t>(3 * found);
        if (int rc = run_kmers<idx_t>(be, a.sa, a.lcp, n, k, min_count, max_count, dRec, found, n_records, w)) return rc;
        be.d2h(records, dRec, found * 24);
        be.sync();
        return CAPS_SA_OK;
    });
}
template <typename idx_t>
int kmer_spectrum_host(const idx_t* SA, const idx_t* LCP, uint64_t n, uint64_t k, uint32_t bins, uint64_t* hist, int device)
{
    if (int rc = check_arrays<idx_t>(n, !SA || !LCP, "null pointer")) return rc;
    if (!hist) return fail(CAPS_SA_EINVAL, "null pointer");
    if (k == 0) return fail(CAPS_SA_EINVAL, "k must be at least 1");
    if (bins < 1 || bins > KMER_MAX_BINS) return fail(CAPS_SA_EINVAL, "bins must be in 1 .. 1024");
    if (n == 0 || k > n) { std::memset(hist, 0, ((size_t)bins + 1) * sizeof(uint64_t)); return CAPS_SA_OK; }
    DeviceScope restore_device_;
    if (int rc = set_device(device)) return rc;
    return guarded([&]() -> int {
        Backend be(nullptr);
        DevAllocs da(be);
        UploadedSaLcp<idx_t> a(be, da, SA, LCP, n);
        return run_kmer_spectrum<idx_t>(be, a.sa, a.lcp, n, k, bins, hist, kmer_ws(da, nullptr, n));
    });
}
template <typename idx_t>
int kmer_census_host(const idx_t* SA, const idx_t* LCP, uint64_t n, uint32_t max_k, uint64_t* distinct, uint64_t* unique, int device)
{
    if (int rc = check_arrays<idx_t>(n, !SA || !LCP, "null pointer")) return rc;
    if (!distinct || !unique) return fail(CAPS_SA_EINVAL, "null pointer");
    if (max_k < 1 || max_k > KMER_MAX_BINS) return fail(CAPS_SA_EINVAL, "max_k must be in 1 .. 1024");
    if (n == 0) {
        std::memset(distinct, 0, ((size_t)max_k + 1) * sizeof(uint64_t));
        std::memset(unique, 0, ((size_t)max_k + 1) * sizeof(uint64_t));
        return CAPS_SA_OK;
    }
    DeviceScope restore_device_;
    if (int rc = set_device(device)) return rc;
    return guarded([&]() -> int {
        Backend be(nullptr);
        DevAllocs da(be);
        UploadedSaLcp<idx_t> a(be, da, SA, LCP, n);
        return run_kmer_census<idx_t>(be, a.sa, a.lcp, n, max_k, distinct, unique, kmer_ws(da, nullptr, n));
    });
}

// ---- k-mers across a collection (include/caps_sa_hip.h "k-mers across a collection"; kernels.h ck_*) -----------------------------------
// Workspace: next[n_tiles + 1] | cnt[n_tiles + 1] | front docs, front occ, carry docs, carry occ [n_tiles] each | the document table[128] |
// totals[CK_COLS] | per-workgroup rows[grid][CK_COLS], 64-bit words.
struct CollPlan {
    uint64_t n_tiles = 0;
    uint32_t grid = 1;                         // workgroups of the sharing kernel (= the length of a column)
    size_t off_next = 0, off_cnt = 0, off_pd = 0, off_po = 0, off_cd = 0, off_co = 0, off_tab = 0, off_tot = 0, off_hist = 0, bytes = 0;
};
inline CollPlan coll_plan(uint64_t n)
{
    CollPlan p;
    p.n_tiles = (n + KMER_TILE - 1) / KMER_TILE;
    p.grid = capped_grid(std::min<uint64_t>(p.n_tiles, 1024), FM_NT);     // (the kernel flushes its 32-bit counters itself)
    const size_t col = align_up((p.n_tiles + 1) * 8);
    p.off_next = 0;
    p.off_cnt = p.off_next + col;
    p.off_pd = p.off_cnt + col;
    p.off_po = p.off_pd + col;
    p.off_cd = p.off_po + col;
    p.off_co = p.off_cd + col;
    p.off_tab = p.off_co + col;
    p.off_tot = p.off_tab + align_up(2 * CK_MAX_DOCS * 8);
    p.off_hist = p.off_tot + align_up((size_t)CK_COLS * 8);
    p.bytes = p.off_hist + align_up((size_t)CK_COLS * p.grid * 8);
    return p;
}
inline int coll_workspace_bytes(uint64_t n, int idx_bytes, uint64_t* bytes)
{
    if (int rc = check_size_query(n, idx_bytes, bytes)) return rc;
    *bytes = ws_reported(coll_plan(n).bytes);
    return CAPS_SA_OK;
}
struct CollWs {
    char* base = nullptr;
    CollPlan p;
    uint64_t* at(size_t off) const { return reinterpret_cast<uint64_t*>(base + off); }
};
inline CollWs coll_ws(DevAllocs& da, void* workspace, uint64_t n)
{
    CollWs w;
    w.p = coll_plan(n);
    w.base = ws_carve(da, workspace, w.p.bytes);
    return w;
}
struct CollDocs { const uint64_t* start; const uint64_t* len; uint32_t m; };

// everything but the outputs: the arrays, k, the documents, the workspace
template <typename idx_t>
int coll_check(const void* SA, const void* LCP, uint64_t n, uint64_t k, const CollDocs& dc, void* workspace, uint64_t workspace_bytes)
{
    if (int rc = check_arrays<idx_t>(n, !SA || !LCP, "null pointer")) return rc;
    if (k == 0) return fail(CAPS_SA_EINVAL, "k must be at least 1");
    if (dc.m < 1 || dc.m > CK_MAX_DOCS) return fail(CAPS_SA_EINVAL, "m must be in 1 .. 64");
    if (!dc.start || !dc.len) return fail(CAPS_SA_EINVAL, "null pointer");
    uint64_t prev_end = 0;
    for (uint32_t d = 0; d < dc.m; ++d) {
        if (dc.len[d] > n || dc.start[d] > n - dc.len[d]) return fail(CAPS_SA_EINVAL, "a document passes the end of the text");
        if (dc.start[d] < prev_end) return fail(CAPS_SA_EINVAL, "the documents must be ascending and disjoint");
        prev_end = dc.start[d] + dc.len[d];
    }
    return ws_check(workspace, workspace_bytes, coll_plan(n).bytes, "workspace too small (caps_sa_hip_coll_workspace_bytes)");
}
inline int coll_check_filter(const CollDocs& dc, const CkFilter& q)
{
    if (q.max_docs && q.min_docs > q.max_docs) return fail(CAPS_SA_EINVAL, "min_docs > max_docs");
    if (q.all_of & q.none_of) return fail(CAPS_SA_EINVAL, "all_of and none_of share a document");
    if (dc.m < 64 && ((q.all_of | q.none_of) >> dc.m)) return fail(CAPS_SA_EINVAL, "a mask names a document at or above m");
    return CAPS_SA_OK;
}

// the table up, then front parts, carries and next[] (1 <= k <= n); `tab` must live until the stream has been synchronised
struct CollTable { uint64_t v[2 * CK_MAX_DOCS]; uint32_t top = 1; };
template <typename idx_t>
void run_coll_edges(Backend& be, const idx_t* dSA, const idx_t* dLCP, uint64_t n, uint64_t k, const CollDocs& dc, CollTable& tab, const CollWs& w)
{
    for (uint32_t d = 0; d < CK_MAX_DOCS; ++d) {
        tab.v[d] = d < dc.m ? dc.start[d] : ~0ull;
        tab.v[CK_MAX_DOCS + d] = d < dc.m ? dc.start[d] + dc.len[d] : 0;
    }
    tab.top = 1;
    while (tab.top < dc.m) tab.top <<= 1;
    be.h2d(w.at(w.p.off_tab), tab.v, sizeof(tab.v));
    const uint32_t tg = capped_grid(std::min<uint64_t>(w.p.n_tiles, 1u << 20), FM_NT);
    CAPS_LAUNCH((ck_edge_kernel<idx_t>), tg, FM_NT, be, dSA, dLCP, n, k, w.p.n_tiles, (const uint64_t*)w.at(w.p.off_tab), tab.top, w.at(w.p.off_next),
                w.at(w.p.off_pd), w.at(w.p.off_po));
    CAPS_LAUNCH(ck_close_kernel, 1, FM_NT, be, (const uint64_t*)w.at(w.p.off_next), (const uint64_t*)w.at(w.p.off_pd),
                (const uint64_t*)w.at(w.p.off_po), w.at(w.p.off_cd), w.at(w.p.off_co), w.p.n_tiles, n);
    CAPS_LAUNCH(kmer_next_kernel, 1, FM_NT, be, w.at(w.p.off_next), w.p.n_tiles, n);
}
template <typename idx_t, int MODE>
void launch_coll_run(Backend& be, uint32_t grid, const idx_t* dSA, const idx_t* dLCP, uint64_t n, uint64_t k, const CollDocs& dc, const CollTable& tab,
                     const CkFilter& q, uint64_t* dRec, uint64_t cap, const CollWs& w)
{
    CAPS_LAUNCH((ck_run_kernel<idx_t, MODE>), grid, FM_NT, be, dSA, dLCP, n, k, w.p.n_tiles, (const uint64_t*)w.at(w.p.off_tab), tab.top, dc.m,
                (const uint64_t*)w.at(w.p.off_next), (const uint64_t*)w.at(w.p.off_cd), (const uint64_t*)w.at(w.p.off_co), q, w.at(w.p.off_cnt),
                dRec, cap, w.at(w.p.off_hist));
}

// the counting call: cnt[] scanned, *found down (1 <= k <= n)
template <typename idx_t>
void run_coll_count(Backend& be, const idx_t* dSA, const idx_t* dLCP, uint64_t n, uint64_t k, const CollDocs& dc, CollTable& tab, const CkFilter& q,
                    uint64_t* found, const CollWs& w)
{
    run_coll_edges<idx_t>(be, dSA, dLCP, n, k, dc, tab, w);
    const uint32_t tg = capped_grid(std::min<uint64_t>(w.p.n_tiles, 1u << 20), FM_NT);
    launch_coll_run<idx_t, CK_COUNT>(be, tg, dSA, dLCP, n, k, dc, tab, q, nullptr, 0, w);
    CAPS_LAUNCH(fm_scan_kernel, 1, FM_NT, be, w.at(w.p.off_cnt), w.p.n_tiles, 0u, 1u, w.at(w.p.off_tot));
    be.d2h(found, w.at(w.p.off_tot), sizeof(uint64_t));
    be.sync();
}
// the writing call, behind run_coll_count on the same workspace
template <typename idx_t>
void run_coll_write(Backend& be, const idx_t* dSA, const idx_t* dLCP, uint64_t n, uint64_t k, const CollDocs& dc, const CollTable& tab,
                    const CkFilter& q, void* dRec, uint64_t capacity, const CollWs& w)
{
    const uint32_t tg = capped_grid(std::min<uint64_t>(w.p.n_tiles, 1u << 20), FM_NT);
    launch_coll_run<idx_t, CK_WRITE>(be, tg, dSA, dLCP, n, k, dc, tab, q, static_cast<uint64_t*>(dRec), capacity, w);
    be.sync();
}
inline void coll_zero_summary(uint64_t* freq, uint64_t* shared, uint32_t m)
{
    std::memset(freq, 0, (CK_MAX_DOCS + 1) * sizeof(uint64_t));
    std::memset(shared, 0, (size_t)m * m * sizeof(uint64_t));
}
template <typename idx_t>
void run_coll_sharing(Backend& be, const idx_t* dSA, const idx_t* dLCP, uint64_t n, uint64_t k, const CollDocs& dc, uint64_t* freq, uint64_t* shared,
                      const CollWs& w)
{
    CollTable tab;
    run_coll_edges<idx_t>(be, dSA, dLCP, n, k, dc, tab, w);
    launch_coll_run<idx_t, CK_SHARING>(be, w.p.grid, dSA, dLCP, n, k, dc, tab, CkFilter{1, 0, 0, 0}, nullptr, 0, w);
    CAPS_LAUNCH(ck_sum_kernel, (CK_COLS + FM_NT - 1) / FM_NT, FM_NT, be, (const uint64_t*)w.at(w.p.off_hist), w.p.grid, w.at(w.p.off_tot));
    std::vector<uint64_t> t(CK_COLS);
    be.d2h(t.data(), w.at(w.p.off_tot), t.size() * sizeof(uint64_t));
    be.sync();
    const uint32_t m = dc.m;
    coll_zero_summary(freq, shared, m);
    for (uint32_t c = 1; c <= m; ++c) freq[c] = t[CK_FREQ + c];
    freq[m] += t[CK_FULL];
    for (uint32_t a = 0; a < m; ++a)
        for (uint32_t b = a; b < m; ++b) shared[(size_t)a * m + b] = shared[(size_t)b * m + a] = t[(size_t)a * CK_MAX_DOCS + b] + t[CK_FULL];
}

template <typename idx_t>
int coll_kmers_device(const void* dSA, const void* dLCP, uint64_t n, uint64_t k, const CollDocs& dc, const CkFilter& q0, void* dRec, uint64_t capacity,
                      uint64_t* n_records, void* workspace, uint64_t workspace_bytes, void* stream)
{
    if (int rc = coll_check<idx_t>(dSA, dLCP, n, k, dc, workspace, workspace_bytes)) return rc;
    if (int rc = coll_check_filter(dc, q0)) return rc;
    if (!n_records) return fail(CAPS_SA_EINVAL, "null pointer");
    if (reinterpret_cast<uintptr_t>(dRec) & 7u) return fail(CAPS_SA_EINVAL, "dRecords must be 8-byte aligned");
    CkFilter q = q0;
    if (q.min_docs == 0) q.min_docs = 1;
    *n_records = 0;
    if (n == 0 || k > n) return CAPS_SA_OK;
    return guarded([&]() -> int {
        Backend be(static_cast<decltype(Backend::stream)>(stream));
        DevAllocs da(be);
        const CollWs w = coll_ws(da, workspace, n);
        const idx_t* sa = static_cast<const idx_t*>(dSA);
        const idx_t* lcp = static_cast<const idx_t*>(dLCP);
        CollTable tab;
        run_coll_count<idx_t>(be, sa, lcp, n, k, dc, tab, q, n_records, w);
        if (!dRec) return CAPS_SA_OK;
        if (*n_records > capacity) return fail(CAPS_SA_EINVAL, "capacity is smaller than the number of records (*n_records; a call with dRecords = NULL counts them)");
        if (*n_records) run_coll_write<idx_t>(be, sa, lcp, n, k, dc, tab, q, dRec, capacity, w);
        return CAPS_SA_OK;
    });
}
template <typename idx_t>
int coll_sharing_device(const void* dSA, const void* dLCP, uint64_t n, uint64_t k, const CollDocs& dc, uint64_t* freq, uint64_t* shared,
                        void* workspace, uint64_t workspace_bytes, void* stream)
{
    if (int rc = coll_check<idx_t>(dSA, dLCP, n, k, dc, workspace, workspace_bytes)) return rc;
    if (!freq || !shared) return fail(CAPS_SA_EINVAL, "null pointer");
    if (n == 0 || k > n) { coll_zero_summary(freq, shared, dc.m); return CAPS_SA_OK; }
    return guarded([&]() -> int {
        Backend be(static_cast<decltype(Backend::stream)>(stream));
        DevAllocs da(be);
        const CollWs w = coll_ws(da, workspace, n);
        run_coll_sharing<idx_t>(be, static_cast<const idx_t*>(dSA), static_cast<const idx_t*>(dLCP), n, k, dc, freq, shared, w);
        return CAPS_SA_OK;
    });
}
template <typename idx_t>
int coll_kmers_host(const idx_t* SA, const idx_t* LCP, uint64_t n, uint64_t k, const CollDocs& dc, const CkFilter& q0, void* records, uint64_t capacity,
                    uint64_t* n_records, int device)
{
    if (int rc = coll_check<idx_t>(SA, LCP, n, k, dc, nullptr, 0)) return rc;
    if (int rc = coll_check_filter(dc, q0)) return rc;
    if (!n_records) return fail(CAPS_SA_EINVAL, "null pointer");
    if (reinterpret_cast<uintptr_t>(records) & 7u) return fail(CAPS_SA_EINVAL, "records must be 8-byte aligned");
    CkFilter q = q0;
    if (q.min_docs == 0) q.min_docs = 1;
    *n_records = 0;
    if (n == 0 || k > n) return CAPS_SA_OK;
    DeviceScope restore_device_;
    if (int rc = set_device(device)) return rc;
    return guarded([&]() -> int {
        Backend be(nullptr);
        DevAllocs da(be);
        UploadedSaLcp<idx_t> a(be, da, SA, LCP, n);
        const CollWs w = coll_ws(da, nullptr, n);
        CollTable tab;
        run_coll_count<idx_t>(be, a.sa, a.lcp, n, k, dc, tab, q, n_records, w);
        if (!records) return CAPS_SA_OK;
        if (*n_records > capacity) return fail(CAPS_SA_EINVAL, "capacity is smaller than the number of records (*n_records; a call with records = NULL counts them)");
        if (*n_records == 0) return CAPS_SA_OK;
        const uint64_t found = *n_records;
        uint64_t* dRec = da.get<uint64_t>(4 * found);
        run_coll_write<idx_t>(be, a.sa, a.lcp, n, k, dc, tab, q, dRec, found, w);
        be.d2h(records, dRec, found * 32);
        be.sync();
        return CAPS_SA_OK;
    });
}
template <typename idx_t>
int coll_sharing_host(const idx_t* SA, const idx_t* LCP, uint64_t n, uint64_t k, const CollDocs& dc, uint64_t* freq, uint64_t* shared, int device)
{
    if (int rc = coll_check<idx_t>(SA, LCP, n, k, dc, nullptr, 0)) return rc;
    if (!freq || !shared) return fail(CAPS_SA_EINVAL, "null pointer");
    if (n == 0 || k > n) { coll_zero_summary(freq, shared, dc.m); return CAPS_SA_OK; }
    DeviceScope restore_device_;
    if (int rc = set_device(device)) return rc;
    return guarded([&]() -> int {
        Backend be(nullptr);
        DevAllocs da(be);
        UploadedSaLcp<idx_t> a(be, da, SA, LCP, n);
        run_coll_sharing<idx_t>(be, a.sa, a.lcp, n, k, dc, freq, shared, coll_ws(da, nullptr, n));
        return CAPS_SA_OK;
    });
}

// ---- MUMs and MEMs between two texts (include/caps_sa_hip.h "MUMs and MEMs between two texts"; kernels.h xm_*) ----------------------------
// Workspace: cnt[XM_KEYS][n_tiles] | tot[XM_KEYS] | lcs[2 * grid] | out[8], 64-bit words.
struct CrossPlan {
    uint64_t n_tiles = 0;
    uint32_t grid = 1;
    size_t off_cnt = 0, off_tot = 0, off_lcs = 0, off_out = 0, bytes = 0;
};
inline CrossPlan cross_plan(uint64_t n)
{
    CrossPlan p;
    p.n_tiles = (n + XM_TILE - 1) / XM_TILE;
    p.grid = capped_grid(std::min<uint64_t>(p.n_tiles, 8192), FM_NT);
    p.off_cnt = 0;
    p.off_tot = p.off_cnt + align_up((XM_KEYS * p.n_tiles + 1) * 8);
    p.off_lcs = p.off_tot + align_up(XM_KEYS * 8);
    p.off_out = p.off_lcs + align_up((size_t)2 * p.grid * 8);
    p.bytes = p.off_out + align_up(8 * 8);
    return p;
}
inline int cross_workspace_bytes(uint64_t n, int idx_bytes, uint64_t* bytes)
{
    if (int rc = check_size_query(n, idx_bytes, bytes)) return rc;
    *bytes = ws_reported(cross_plan(n).bytes);
    return CAPS_SA_OK;
}
struct CrossWs {
    char* base = nullptr;
    CrossPlan p;
    uint64_t* cnt() const { return reinterpret_cast<uint64_t*>(base + p.off_cnt); }
    uint64_t* tot() const { return reinterpret_cast<uint64_t*>(base + p.off_tot); }
    uint64_t* lcs() const { return reinterpret_cast<uint64_t*>(base + p.off_lcs); }
    uint64_t* out() const { return reinterpret_cast<uint64_t*>(base + p.off_out); }
};
inline CrossWs cross_ws(DevAllocs& da, void* workspace, uint64_t n)
{
    CrossWs w;
    w.p = cross_plan(n);
    w.base = ws_carve(da, workspace, w.p.bytes);
    return w;
}
// every refusal that needs no device; max_occ = 0 is MUM mode
template <typename idx_t>
int cross_check(const void* SA, const void* LCP, const void* BWT, uint64_t n, uint64_t split, uint64_t min_len, bool mems, uint32_t max_occ,
                const void* records, const uint64_t* summary, void* workspace, uint64_t workspace_bytes)
{
    if (int rc = check_arrays<idx_t>(n, !SA || !LCP || !BWT, "null pointer")) return rc;
    if (!summary) return fail(CAPS_SA_EINVAL, "null pointer");
    if (min_len == 0) return fail(CAPS_SA_EINVAL, "min_len must be at least 1");
    if (split > n) return fail(CAPS_SA_EINVAL, "split is beyond the text (split <= n)");
    if (mems && (max_occ < 2 || max_occ > XM_MAX_OCC)) return fail(CAPS_SA_EINVAL, "max_occ must be in 2 .. 64");
    if (reinterpret_cast<uintptr_t>(records) & 7u) return fail(CAPS_SA_EINVAL, "the records must be 8-byte aligned");
    return ws_check(workspace, workspace_bytes, cross_plan(n).bytes, "workspace too small (caps_sa_hip_cross_workspace_bytes)");
}

// the counting pass: the 8 summary words (n >= 1)
template <typename idx_t>
void run_cross_count(Backend& be, const idx_t* dSA, const idx_t* dLCP, const uint8_t* dBWT, uint64_t n, uint64_t split, uint64_t min_len,
                     uint32_t max_occ, uint64_t* summary, const CrossWs& w)
{
    if (max_occ)
        CAPS_LAUNCH((xm_kernel<idx_t, XM_COUNT, true>), w.p.grid, FM_NT, be, dSA, dLCP, dBWT, n, split, min_len, max_occ, w.p.n_tiles, w.cnt(),
                    w.lcs(), (uint64_t*)nullptr, (uint64_t)0);
    else
        CAPS_LAUNCH((xm_kernel<idx_t, XM_COUNT, false>), w.p.grid, FM_NT, be, dSA, dLCP, dBWT, n, split, min_len, max_occ, w.p.n_tiles, w.cnt(),
                    w.lcs(), (uint64_t*)nullptr, (uint64_t)0);
    CAPS_LAUNCH(fm_scan_kernel, XM_KEYS, FM_NT, be, w.cnt(), w.p.n_tiles, 0u, XM_KEYS, w.tot());
    CAPS_LAUNCH((xm_finish_kernel<idx_t>), 1, FM_NT, be, dSA, n, split, (const uint64_t*)w.lcs(), w.p.grid, (const uint64_t*)w.tot(), w.out());
    be.d2h(summary, w.out(), 8 * sizeof(uint64_t));
    be.sync();
}
// the writing pass behind a counting pass on the same workspace: summary[0] records, at most `capacity` of them stored
template <typename idx_t>
void run_cross_write(Backend& be, const idx_t* dSA, const idx_t* dLCP, const uint8_t* dBWT, uint64_t n, uint64_t split, uint64_t min_len,
                     uint32_t max_occ, void* dRec, uint64_t capacity, const CrossWs& w)
{
    if (max_occ)
        CAPS_LAUNCH((xm_kernel<idx_t, XM_WRITE, true>), w.p.grid, FM_NT, be, dSA, dLCP, dBWT, n, split, min_len, max_occ, w.p.n_tiles, w.cnt(),
                    (uint64_t*)nullptr, static_cast<uint64_t*>(dRec), capacity);
    else
        CAPS_LAUNCH((xm_kernel<idx_t, XM_WRITE, false>), w.p.grid, FM_NT, be, dSA, dLCP, dBWT, n, split, min_len, max_occ, w.p.n_tiles, w.cnt(),
                    (uint64_t*)nullptr, static_cast<uint64_t*>(dRec), capacity);
    be.sync();
}
inline const char* cross_capacity_msg() { return "capacity is smaller than the number of records (summary[0]; a call with the records NULL counts them)"; }

template <typename idx_t>
int cross_device(const void* dSA, const void* dLCP, const void* dBWT, uint64_t n, uint64_t split, uint64_t min_len, bool mems, uint32_t max_occ,
                 void* dRec, uint64_t capacity, uint64_t* summary, void* workspace, uint64_t workspace_bytes, void* stream)
{
    if (int rc = cross_check<idx_t>(dSA, dLCP, dBWT, n, split, min_len, mems, max_occ, dRec, summary, workspace, workspace_bytes)) return rc;
    std::memset(summary, 0, 8 * sizeof(uint64_t));
    if (n == 0) return CAPS_SA_OK;
    if (!mems) max_occ = 0;
    return guarded([&]() -> int {
        Backend be(static_cast<decltype(Backend::stream)>(stream));
        DevAllocs da(be);
        const CrossWs w = cross_ws(da, workspace, n);
        const idx_t* sa = static_cast<const idx_t*>(dSA);
        const idx_t* lcp = static_cast<const idx_t*>(dLCP);
        const uint8_t* bwt = static_cast<const uint8_t*>(dBWT);
        run_cross_count<idx_t>(be, sa, lcp, bwt, n, split, min_len, max_occ, summary, w);
        if (!dRec) return CAPS_SA_OK;
        if (summary[0] > capacity) return fail(CAPS_SA_EINVAL, cross_capacity_msg());
        if (summary[0]) run_cross_write<idx_t>(be, sa, lcp, bwt, n, split, min_len, max_occ, dRec, capacity, w);
        return CAPS_SA_OK;
    });
}
// host arrays: up into buffers of the call's own, the device form on them, the records down
template <typename idx_t>
int cross_host(const idx_t* SA, const idx_t* LCP, const uint8_t* BWT, uint64_t n, uint64_t split, uint64_t min_len, bool mems, uint32_t max_occ,
               void* records, uint64_t capacity, uint64_t* summary, int device)
{
    if (int rc = cross_check<idx_t>(SA, LCP, BWT, n, split, min_len, mems, max_occ, records, summary, nullptr, 0)) return rc;
    std::memset(summary, 0, 8 * sizeof(uint64_t));
    if (n == 0) return CAPS_SA_OK;
    if (!mems) max_occ = 0;
    DeviceScope restore_device_;
    if (int rc = set_device(device)) return rc;
    return guarded([&]() -> int {
        Backend be(nullptr);
        DevAllocs da(be);
        UploadedSaLcp<idx_t> a(be, da, SA, LCP, n);
        uint8_t* bwt = da.get<uint8_t>(n);
        be.h2d(bwt, BWT, n);
        const CrossWs w = cross_ws(da, nullptr, n);
        run_cross_count<idx_t>(be, a.sa, a.lcp, bwt, n, split, min_len, max_occ, summary, w);
        if (!records) return CAPS_SA_OK;
        if (summary[0] > capacity) return fail(CAPS_SA_EINVAL, cross_capacity_msg());
        if (summary[0] == 0) return CAPS_SA_OK;
        const uint64_t found = summary[0];
        uint64_t* dRec = da.get<uint64_t>(3 * found);
        run_cross_write<idx_t>(be, a.sa, a.lcp, bwt, n, split, min_len, max_occ, dRec, found, w);
        be.d2h(records, dRec, found * 24);
        be.sync();
        return CAPS_SA_OK;
    });
}

// ---- LPF and LZ77 from SA and LCP (include/caps_sa_hip.h "LPF and LZ77 from SA and LCP"; kernels.h lpf_* / lz_*) ------------------------
// lpf workspace: tab[2 * LPF_MAX_LEVELS + 2] (offset, nodes of every level) | bad | sumSA[nodes] | sumLCP[nodes], nodes = all levels.
struct LpfPlan {
    uint64_t n_tiles = 0, nodes = 0;
    uint32_t top = 0;                                      // the level that is one node
    uint64_t tab[2 * LPF_MAX_LEVELS + 2] = {};
    size_t off_tab = 0, off_bad = 0, off_sa = 0, off_lcp = 0, bytes = 0;
};
inline LpfPlan lpf_plan(uint64_t n, size_t w)
{
    LpfPlan p;
    p.n_tiles = (n + LPF_TILE - 1) / LPF_TILE;
    uint64_t cnt = n;
    do {
        cnt = (cnt + LPF_F - 1) / LPF_F;
        ++p.top;
        p.tab[2 * p.top] = p.nodes;
        p.tab[2 * p.top + 1] = cnt;
        p.nodes += cnt;
    } while (cnt > 1 && p.top + 1 < LPF_MAX_LEVELS);
    p.off_tab = 0;
    p.off_bad = align_up(sizeof(p.tab));
    p.off_sa = p.off_bad + WS_ALIGN;
    p.off_lcp = p.off_sa + align_up(p.nodes * w);
    p.bytes = p.off_lcp + align_up(p.nodes * w);
    return p;
}
// lz77 workspace: ex[n] | gx[n_groups * LZ_SPEC] (index width) | gentry[n_groups] | entry[n_tiles] | cnt[n_tiles + 1] | total, 64-bit words
struct LzPlan {
    uint64_t n_tiles = 0, n_groups = 0;
    size_t off_ex = 0, off_gx = 0, off_gentry = 0, off_entry = 0, off_cnt = 0, off_tot = 0, bytes = 0;
};
inline LzPlan lz_plan(uint64_t n, size_t w)
{
    LzPlan p;
    p.n_tiles = (n + LZ_TILE - 1) / LZ_TILE;
    p.n_groups = (n + LZ_GPOS - 1) / LZ_GPOS;
    p.off_ex = 0;
    p.off_gx = align_up(n * w);
    p.off_gentry = p.off_gx + align_up(p.n_groups * LZ_SPEC * w);
    p.off_entry = p.off_gentry + align_up(p.n_groups * 8);
    p.off_cnt = p.off_entry + align_up(p.n_tiles * 8);
    p.off_tot = p.off_cnt + align_up((p.n_tiles + 1) * 8);
    p.bytes = p.off_tot + WS_ALIGN;
    return p;
}
inline int lpf_workspace_bytes(uint64_t n, int idx_bytes, uint64_t* bytes)
{
    if (int rc = check_size_query(n, idx_bytes, bytes)) return rc;
    *bytes = ws_reported(lpf_plan(n, (size_t)idx_bytes).bytes);
    return CAPS_SA_OK;
}
inline int lz77_workspace_bytes(uint64_t n, int idx_bytes, uint64_t* bytes)
{
    if (int rc = check_size_query(n, idx_bytes, bytes)) return rc;
    *bytes = ws_reported(lz_plan(n, (size_t)idx_bytes).bytes);
    return CAPS_SA_OK;
}

// n >= 1, dLPF or dPrev non-null
template <typename idx_t>
int run_lpf(Backend& be, const idx_t* dSA, const idx_t* dLCP, uint64_t n, idx_t* dLPF, idx_t* dPrev, char* ws)
{
    const LpfPlan p = lpf_plan(n, sizeof(idx_t));
    uint64_t* tab = reinterpret_cast<uint64_t*>(ws + p.off_tab);
    uint32_t* bad = reinterpret_cast<uint32_t*>(ws + p.off_bad);
    idx_t* sumSA = reinterpret_cast<idx_t*>(ws + p.off_sa);
    idx_t* sumLCP = reinterpret_cast<idx_t*>(ws + p.off_lcp);
    be.h2d(tab, p.tab, sizeof(p.tab));
    be.memset(bad, 0, sizeof(uint32_t));
    const uint32_t tg = capped_grid(std::min<uint64_t>(p.n_tiles, 1u << 20), FM_NT);
    CAPS_LAUNCH((lpf_block_kernel<idx_t>), tg, FM_NT, be, dSA, dLCP, n, p.n_tiles, p.tab[3], sumSA, sumLCP);
    for (uint32_t lev = 2; lev <= p.top; ++lev) {
        const uint64_t n_par = p.tab[2 * lev + 1];
        const uint32_t g = capped_grid(std::min<uint64_t>((n_par + FM_NT - 1) / FM_NT, 1u << 16), FM_NT);
        CAPS_LAUNCH((lpf_up_kernel<idx_t>), g, FM_NT, be, sumSA, sumLCP, p.tab[2 * lev - 2], p.tab[2 * lev - 1], p.tab[2 * lev], n_par);
    }
    CAPS_LAUNCH((lpf_tile_kernel<idx_t>), tg, FM_NT, be, dSA, dLCP, n, p.n_tiles, p.tab[3], (const idx_t*)sumSA, (const idx_t*)sumLCP,
                (const uint64_t*)tab, p.top, dLPF, dPrev, bad);
    uint32_t is_bad = 0;
    be.d2h(&is_bad, bad, sizeof(uint32_t));
    be.sync();
    if (is_bad) return fail(CAPS_SA_EINVAL, "not a suffix array: a value of SA is n or more");
    return CAPS_SA_OK;
}

// the parse of (dLPF, dPrev): *found always; with dRec the records.  counted: the workspace still holds entry[] and the scanned
// cnt[] of a counting call on the same arrays (the host form's second call), and *found its result.
template <typename idx_t>
int run_lz77(Backend& be, const idx_t* dLPF, const idx_t* dPrev, uint64_t n, void* dRec, uint64_t capacity, uint64_t* found, char* ws,
             bool counted = false)
{
    if (!counted) *found = 0;
    if (n == 0) return CAPS_SA_OK;
    const LzPlan p = lz_plan(n, sizeof(idx_t));
    idx_t* ex = reinterpret_cast<idx_t*>(ws + p.off_ex);
    idx_t* gx = reinterpret_cast<idx_t*>(ws + p.off_gx);
    uint64_t* gentry = reinterpret_cast<uint64_t*>(ws + p.off_gentry);
    uint64_t* entry = reinterpret_cast<uint64_t*>(ws + p.off_entry);
    uint64_t* cnt = reinterpret_cast<uint64_t*>(ws + p.off_cnt);
    uint64_t* tot = reinterpret_cast<uint64_t*>(ws + p.off_tot);
    const uint32_t tg = capped_grid(std::min<uint64_t>(p.n_tiles, 1u << 20), FM_NT);
    if (!counted) {
        CAPS_LAUNCH((lz_exit_kernel<idx_t>), tg, FM_NT, be, dLPF, n, p.n_tiles, ex);
        const uint32_t gg = capped_grid(std::min<uint64_t>((p.n_groups * LZ_SPEC + FM_NT - 1) / FM_NT, 1u << 16), FM_NT);
        CAPS_LAUNCH((lz_group_kernel<idx_t>), gg, FM_NT, be, (const idx_t*)ex, n, p.n_groups, gx);
        CAPS_LAUNCH((lz_hop_kernel<idx_t>), 1, FM_NT, be, (const idx_t*)ex, (const idx_t*)gx, n, p.n_groups, gentry);
        const uint32_t eg = capped_grid(std::min<uint64_t>((p.n_groups + FM_NT - 1) / FM_NT, 1u << 16), FM_NT);
        CAPS_LAUNCH((lz_entry_kernel<idx_t>), eg, FM_NT, be, (const idx_t*)ex, n, p.n_tiles, p.n_groups, (const uint64_t*)gentry, entry);
        CAPS_LAUNCH((lz_walk_kernel<idx_t, LZ_COUNT>), tg, FM_NT, be, dLPF, dPrev, n, p.n_tiles, (const uint64_t*)entry, cnt, (uint64_t*)nullptr,
                    (uint64_t)0);
        CAPS_LAUNCH(fm_scan_kernel, 1, FM_NT, be, cnt, p.n_tiles, 0u, 1u, tot);
        be.d2h(found, tot, sizeof(uint64_t));
        be.sync();
    }
    if (!dRec) return CAPS_SA_OK;
    if (*found > capacity) return fail(CAPS_SA_EINVAL, "capacity is smaller than the number of phrases (*n_phrases; a call with dRecords = NULL counts them)");
    CAPS_LAUNCH((lz_walk_kernel<idx_t, LZ_WRITE>), tg, FM_NT, be, dLPF, dPrev, n, p.n_tiles, (const uint64_t*)entry, cnt,
                static_cast<uint64_t*>(dRec), capacity);
    be.sync();
    return CAPS_SA_OK;
}

template <typename idx_t>
int lpf_device(const void* dSA, const void* dLCP, uint64_t n, void* dLPF, void* dPrev, void* workspace, uint64_t workspace_bytes, void* stream)
{
    if (int rc = check_arrays<idx_t>(n, !dSA || !dLCP, "dSA or dLCP is null")) return rc;
    if (n && !dLPF && !dPrev) return fail(CAPS_SA_EINVAL, "dLPF and dPrev are both null");
    if (int rc = ws_check(workspace, workspace_bytes, lpf_plan(n, sizeof(idx_t)).bytes, "workspace too small (caps_sa_hip_lpf_workspace_bytes)")) return rc;
    if (n == 0) return CAPS_SA_OK;
    return guarded([&]() -> int {
        Backend be(static_cast<decltype(Backend::stream)>(stream));
        DevAllocs da(be);
        char* ws = ws_carve(da, workspace, lpf_plan(n, sizeof(idx_t)).bytes);
        return run_lpf<idx_t>(be, static_cast<const idx_t*>(dSA), static_cast<const idx_t*>(dLCP), n, static_cast<idx_t*>(dLPF),
                              static_cast<idx_t*>(dPrev), ws);
    });
}
template <typename idx_t>
int lz77_device(const void* dLPF, const void* dPrev, uint64_t n, void* dRec, uint64_t capacity, uint64_t* n_phrases, void* workspace,
                uint64_t workspace_bytes, void* stream)
{
    if (int rc = check_arrays<idx_t>(n, !dLPF || !dPrev, "dLPF or dPrev is null")) return rc;
    if (!n_phrases) return fail(CAPS_SA_EINVAL, "n_phrases is null");
    if (reinterpret_cast<uintptr_t>(dRec) & 7u) return fail(CAPS_SA_EINVAL, "dRecords must be 8-byte aligned");
    if (int rc = ws_check(workspace, workspace_bytes, lz_plan(n, sizeof(idx_t)).bytes, "workspace too small (caps_sa_hip_lz77_workspace_bytes)")) return rc;
    if (n == 0) { *n_phrases = 0; return CAPS_SA_OK; }
    return guarded([&]() -> int {
        Backend be(static_cast<decltype(Backend::stream)>(stream));
        DevAllocs da(be);
        char* ws = ws_carve(da, workspace, lz_plan(n, sizeof(idx_t)).bytes);
        return run_lz77<idx_t>(be, static_cast<const idx_t*>(dLPF), static_cast<const idx_t*>(dPrev), n, dRec, capacity, n_phrases, ws);
    });
}
template <typename idx_t>
int lpf_host(const idx_t* SA, const idx_t* LCP, uint64_t n, idx_t* LPF, idx_t* Prev, int device)
{
    if (int rc = check_arrays<idx_t>(n, !SA || !LCP, "SA or LCP is null")) return rc;
    if (n && !LPF && !Prev) return fail(CAPS_SA_EINVAL, "LPF and Prev are both null");
    if (n == 0) return CAPS_SA_OK;
    DeviceScope restore_device_;
    if (int rc = set_device(device)) return rc;
    return guarded([&]() -> int {
        Backend be(nullptr);
        DevAllocs da(be);
        UploadedSaLcp<idx_t> a(be, da, SA, LCP, n);
        idx_t* dLPF = LPF ? da.get<idx_t>(n) : nullptr;
        idx_t* dPrev = Prev ? da.get<idx_t>(n) : nullptr;
        // slots whose position never occurs in SA keep what they held
        if (LPF) be.h2d(dLPF, LPF, n * sizeof(idx_t));
        if (Prev) be.h2d(dPrev, Prev, n * sizeof(idx_t));
        char* ws = ws_carve(da, nullptr, lpf_plan(n, sizeof(idx_t)).bytes);
        const int rc = run_lpf<idx_t>(be, a.sa, a.lcp, n, dLPF, dPrev, ws);
        if (LPF) be.d2h(LPF, dLPF, n * sizeof(idx_t));
        if (Prev) be.d2h(Prev, dPrev, n * sizeof(idx_t));
        be.sync();
        return rc;
    });
}
template <typename idx_t>
int lz77_host(const idx_t* SA, const idx_t* LCP, uint64_t n, void* records, uint64_t capacity, uint64_t* n_phrases, int device)
{
    if (int rc = check_arrays<idx_t>(n, !SA || !LCP, "SA or LCP is null")) return rc;
    if (!n_phrases) return fail(CAPS_SA_EINVAL, "n_phrases is null");
    if (reinterpret_cast<uintptr_t>(records) & 7u) return fail(CAPS_SA_EINVAL, "records must be 8-byte aligned");
    if (n == 0) { *n_phrases = 0; return CAPS_SA_OK; }
    DeviceScope restore_device_;
    if (int rc = set_device(device)) return rc;
    return guarded([&]() -> int {
        Backend be(nullptr);
        DevAllocs da(be);
        UploadedSaLcp<idx_t> a(be, da, SA, LCP, n);
        idx_t* dLPF = da.get<idx_t>(n);
        idx_t* dPrev = da.get<idx_t>(n);
        be.memset(dLPF, 0, n * sizeof(idx_t));              // a position that SA never names parses as a literal
        be.memset(dPrev, 0xFF, n * sizeof(idx_t));
        char* ws = ws_carve(da, nullptr, std::max(lpf_plan(n, sizeof(idx_t)).bytes, lz_plan(n, sizeof(idx_t)).bytes));
        if (int rc = run_lpf<idx_t>(be, a.sa, a.lcp, n, dLPF, dPrev, ws)) return rc;
        if (int rc = run_lz77<idx_t>(be, dLPF, dPrev, n, nullptr, 0, n_phrases, ws)) return rc;
        if (!records) return CAPS_SA_OK;
        if (*n_phrases > capacity) return fail(CAPS_SA_EINVAL, "capacity is smaller than the number of phrases (*n_phrases; a call with records = NULL counts them)");
        const uint64_t found = *n_phrases;
        uint64_t* dRec = da.get<uint64_t>(3 * found);
        if (int rc = run_lz77<idx_t>(be, dLPF, dPrev, n, dRec, found, n_phrases, ws, true)) return rc;    // entry[] and cnt[] are still there
        be.d2h(records, dRec, found * 24);
        be.sync();
        return CAPS_SA_OK;
    });
}

// ---- ISA and the LCE index (include/caps_sa_hip.h "ISA and longest common extensions"; kernels.h isa_* / lce_*) -----------------------
// The blob: a header of LCE_HDR_WORDS 64-bit words, then ISA[n] | LCP[n] | M_0 .. M_6 (nb entries each) | T_0 .. T_{tlevels-1} (ns
// entries each), every array rounded up to 256 bytes.  Every header word follows from n and the index width.
constexpr uint64_t LCE_MAGIC = 0x3145434C53504143ull;     // "CAPSLCE1"
constexpr uint64_t LCE_VERSION = 1;
constexpr uint32_t LCE_HDR_WORDS = 32;
static_assert(LCE_HDR_WORDS == FM_HDR_WORDS, "blob_mark_resident keeps a header of this size and sums the body behind it");
enum { LCEH_MAGIC = 0, LCEH_VERSION, LCEH_N, LCEH_IDX_BYTES, LCEH_BLOCK, LCEH_SUPER, LCEH_NB, LCEH_NS, LCEH_TLEVELS, LCEH_OFF_ISA, LCEH_OFF_LCP,
       LCEH_OFF_M, LCEH_M_STRIDE, LCEH_OFF_T, LCEH_T_STRIDE, LCEH_TOTAL };

struct LceLayout {
    uint64_t nb = 0, ns = 0, tlevels = 0, off_isa = 0, off_lcp = 0, off_m = 0, m_stride = 0, off_t = 0, t_stride = 0, total = 0;
};
inline LceLayout lce_layout(uint64_t n, uint64_t w)
{
    LceLayout l;
    l.nb = (n + LCE_BLOCK - 1) / LCE_BLOCK;
    l.ns = (n + LCE_SUPER - 1) / LCE_SUPER;
    l.tlevels = l.ns ? 64u - (uint64_t)caps_clz64(l.ns) : 0;          // floor(log2 ns) + 1
    l.off_isa = LCE_HDR_WORDS * sizeof(uint64_t);
    l.off_lcp = l.off_isa + align_up(n * w);
    l.off_m = l.off_lcp + align_up(n * w);
    l.m_stride = align_up(l.nb * w);
    l.off_t = l.off_m + LCE_MLEVELS * l.m_stride;
    l.t_stride = align_up(l.ns * w);
    l.total = l.off_t + l.tlevels * l.t_stride;
    return l;
}
inline void lce_header(uint64_t* h, uint64_t n, uint64_t w)
{
    const LceLayout l = lce_layout(n, w);
    std::memset(h, 0, LCE_HDR_WORDS * sizeof(uint64_t));
    h[LCEH_MAGIC] = LCE_MAGIC; h[LCEH_VERSION] = LCE_VERSION; h[LCEH_N] = n; h[LCEH_IDX_BYTES] = w; h[LCEH_BLOCK] = LCE_BLOCK;
    h[LCEH_SUPER] = LCE_SUPER; h[LCEH_NB] = l.nb; h[LCEH_NS] = l.ns; h[LCEH_TLEVELS] = l.tlevels; h[LCEH_OFF_ISA] = l.off_isa;
    h[LCEH_OFF_LCP] = l.off_lcp; h[LCEH_OFF_M] = l.off_m; h[LCEH_M_STRIDE] = l.m_stride; h[LCEH_OFF_T] = l.off_t; h[LCEH_T_STRIDE] = l.t_stride;
    h[LCEH_TOTAL] = l.total;
}
inline int lce_index_bytes(uint64_t n, int idx_bytes, uint64_t* bytes)
{
    if (int rc = check_size_query(n, idx_bytes, bytes)) return rc;
    *bytes = lce_layout(n, (uint64_t)idx_bytes).total;
    return CAPS_SA_OK;
}
// the header, checked on the host before any kernel reads the body: every word is recomputed from n and the index width
inline int lce_check_header(const uint64_t* h, uint64_t index_bytes, const void* dIndex, LceView& v)
{
    if (h[LCEH_MAGIC] != LCE_MAGIC) return fail(CAPS_SA_EINVAL, "not an LCE index of this library (wrong magic)");
    if (h[LCEH_VERSION] != LCE_VERSION) return fail(CAPS_SA_EINVAL, "LCE index of another format version");
    const uint64_t w = h[LCEH_IDX_BYTES], n = h[LCEH_N];
    if (w != 4 && w != 8) return fail(CAPS_SA_EINVAL, "LCE index header: bad index width");
    if ((w == 4 && n > 0xFFFFFFFFull) || n > (1ull << 60)) return fail(CAPS_SA_EINVAL, "LCE index header: n does not fit its index width");
    uint64_t want[LCE_HDR_WORDS];
    lce_header(want, n, w);
    if (std::memcmp(want, h, sizeof want) != 0) return fail(CAPS_SA_EINVAL, "LCE index header: a word does not follow from n and the index width");
    if (want[LCEH_TOTAL] > index_bytes) return fail(CAPS_SA_EINVAL, "index_bytes is smaller than the LCE index (truncated blob)");
    const LceLayout l = lce_layout(n, w);
    const char* base = static_cast<const char*>(dIndex);
    v.n = n; v.nb = l.nb; v.ns = l.ns; v.tlevels = (uint32_t)l.tlevels;
    v.isa = base + l.off_isa; v.lcp = base + l.off_lcp; v.m = base + l.off_m; v.t = base + l.off_t;
    v.m_stride = l.m_stride; v.t_stride = l.t_stride;
    return CAPS_SA_OK;
}
inline int lce_check_blob_args(const void* index, uint64_t index_bytes)
{
    if (!index) return fail(CAPS_SA_EINVAL, "null index");
    if (reinterpret_cast<uintptr_t>(index) & 15u) return fail(CAPS_SA_EINVAL, "the index must be 16-byte aligned");
    if (index_bytes < LCE_HDR_WORDS * sizeof(uint64_t)) return fail(CAPS_SA_EINVAL, "index_bytes is smaller than an LCE index header");
    return CAPS_SA_OK;
}

// n >= 1.  dISA is overwritten whatever SA holds; flags: a device word of the call
template <typename idx_t> int run_isa(Backend& be, const idx_t* dSA, uint64_t n, idx_t* dISA, uint32_t* flags)
{
    constexpr uint32_t PER = 16u / sizeof(idx_t);
    const uint32_t g = capped_grid(std::min<uint64_t>(((n + PER - 1) / PER + FM_NT - 1) / FM_NT, 1u << 16), FM_NT);
    be.memset(flags, 0, sizeof(uint32_t));
    be.memset(dISA, 0xFF, n * sizeof(idx_t));
    CAPS_LAUNCH((isa_scatter_kernel<idx_t>), g, FM_NT, be, dSA, n, dISA, flags);
    CAPS_LAUNCH((isa_check_kernel<idx_t>), g, FM_NT, be, (const idx_t*)dISA, n, flags);
    uint32_t f = 0;
    be.d2h(&f, flags, sizeof f);
    be.sync();
    if (f & 1u) return fail(CAPS_SA_EINVAL, "not a suffix array: a value of SA is n or more");
    if (f & 2u) return fail(CAPS_SA_EINVAL, "not a suffix array: a position occurs twice and another never");
    return CAPS_SA_OK;
}

// the blob of (dSA, dLCP) at dIndex (room for lce_layout(n).total bytes); no workspace beyond it
template <typename idx_t> int run_lce_build(Backend& be, const idx_t* dSA, const idx_t* dLCP, uint64_t n, char* dIndex)
{
    constexpr uint64_t w = sizeof(idx_t);
    const LceLayout l = lce_layout(n, w);
    uint64_t h[LCE_HDR_WORDS];
    lce_header(h, n, w);
    be.h2d(dIndex, h, sizeof h);
    if (n == 0) { be.sync(); return CAPS_SA_OK; }
    auto pad = [&](uint64_t off, uint64_t bytes) {                  // the section's padding is zero: equal inputs, equal blobs
        const uint64_t end = align_up(bytes);
        if (end > bytes) be.memset(dIndex + off + bytes, 0, end - bytes);
    };
    pad(l.off_isa, n * w);
    pad(l.off_lcp, n * w);
    for (uint64_t j = 0; j < LCE_MLEVELS; ++j) pad(l.off_m + j * l.m_stride, l.nb * w);
    for (uint64_t j = 0; j < l.tlevels; ++j) pad(l.off_t + j * l.t_stride, l.ns * w);
    uint32_t* flags = reinterpret_cast<uint32_t*>(call_words(be));
    if (int rc = run_isa<idx_t>(be, dSA, n, reinterpret_cast<idx_t*>(dIndex + l.off_isa), flags)) { be.sync(); return rc; }
    auto M = [&](uint64_t j) { return reinterpret_cast<idx_t*>(dIndex + l.off_m + j * l.m_stride); };
    auto T = [&](uint64_t j) { return reinterpret_cast<idx_t*>(dIndex + l.off_t + j * l.t_stride); };
    auto grid = [](uint64_t lanes) { return capped_grid(std::min<uint64_t>((lanes + FM_NT - 1) / FM_NT, 1u << 16), FM_NT); };
    CAPS_LAUNCH((lce_block_kernel<idx_t>), capped_grid(std::min<uint64_t>(l.ns, 1u << 20), FM_NT), FM_NT, be, dLCP, n, l.ns, l.nb,
                reinterpret_cast<idx_t*>(dIndex + l.off_lcp), M(0));
    for (uint64_t j = 1; j < LCE_MLEVELS; ++j)
        CAPS_LAUNCH((lce_table_kernel<idx_t>), grid(l.nb), FM_NT, be, (const idx_t*)M(j - 1), l.nb, M(j), l.nb, (uint64_t)1, (uint64_t)1 << (j - 1));
    CAPS_LAUNCH((lce_table_kernel<idx_t>), grid(l.ns), FM_NT, be, (const idx_t*)M(LCE_MLEVELS - 1), l.nb, T(0), l.ns, (uint64_t)LCE_BPS, (uint64_t)0);
    for (uint64_t j = 1; j < l.tlevels; ++j)
        CAPS_LAUNCH((lce_table_kernel<idx_t>), grid(l.ns), FM_NT, be, (const idx_t*)T(j - 1), l.ns, T(j), l.ns, (uint64_t)1, (uint64_t)1 << (j - 1));
    be.sync();
    return CAPS_SA_OK;
}

template <typename idx_t> int isa_check_args(const void* SA, uint64_t n, const void* ISA)
{
    return check_arrays<idx_t>(n, !SA || !ISA, "SA or ISA is null");
}
template <typename idx_t> int isa_device(const void* dSA, uint64_t n, void* dISA, void* stream)
{
    if (int rc = isa_check_args<idx_t>(dSA, n, dISA)) return rc;
    if (n == 0) return CAPS_SA_OK;
    return guarded([&]() -> int {
        Backend be(static_cast<decltype(Backend::stream)>(stream));
        return run_isa<idx_t>(be, static_cast<const idx_t*>(dSA), n, static_cast<idx_t*>(dISA), reinterpret_cast<uint32_t*>(call_words(be)));
    });
}
template <typename idx_t> int isa_host(const idx_t* SA, uint64_t n, idx_t* ISA, int device)
{
    if (int rc = isa_check_args<idx_t>(SA, n, ISA)) return rc;
    if (n == 0) return CAPS_SA_OK;
    DeviceScope restore_device_;
    if (int rc = set_device(device)) return rc;
    return guarded([&]() -> int {
        HostPathCache& hc = host_cache();
        std::lock_guard<std::mutex> lock(hc.mu);
        Backend be(nullptr);
        hc.blob_host = nullptr;
        const size_t off_isa = align_up(n * sizeof(idx_t));
        host_block(hc, be, device, off_isa + align_up(n * sizeof(idx_t)));
        idx_t* dSA = reinterpret_cast<idx_t*>(hc.base);
        idx_t* dISA = reinterpret_cast<idx_t*>(hc.base + off_isa);
        be.h2d(dSA, SA, n * sizeof(idx_t));
        if (int rc = run_isa<idx_t>(be, dSA, n, dISA, reinterpret_cast<uint32_t*>(call_words(be)))) return rc;      // ISA is not written
        be.d2h(ISA, dISA, n * sizeof(idx_t));
        be.sync();
        return CAPS_SA_OK;
    });
}

template <typename idx_t> int lce_check_build(const void* SA, const void* LCP, uint64_t n, const void* index, uint64_t index_bytes)
{
    if (int rc = check_arrays<idx_t>(n, !SA || !LCP, "SA or LCP is null")) return rc;
    if (!index) return fail(CAPS_SA_EINVAL, "null index");
    if (reinterpret_cast<uintptr_t>(index) & 15u) return fail(CAPS_SA_EINVAL, "the index must be 16-byte aligned");
    if (index_bytes < lce_layout(n, sizeof(idx_t)).total) return fail(CAPS_SA_EINVAL, "index_bytes too small (caps_sa_hip_lce_index_bytes)");
    return CAPS_SA_OK;
}
template <typename idx_t> int lce_build_device(const void* dSA, const void* dLCP, uint64_t n, void* dIndex, uint64_t index_bytes, void* stream)
{
    if (int rc = lce_check_build<idx_t>(dSA, dLCP, n, dIndex, index_bytes)) return rc;
    return guarded([&]() -> int {
        Backend be(static_cast<decltype(Backend::stream)>(stream));
        return run_lce_build<idx_t>(be, static_cast<const idx_t*>(dSA), static_cast<const idx_t*>(dLCP), n, static_cast<char*>(dIndex));
    });
}
template <typename idx_t> int lce_build_host(const idx_t* SA, const idx_t* LCP, uint64_t n, void* index, uint64_t index_bytes, int device)
{
    if (int rc = lce_check_build<idx_t>(SA, LCP, n, index, index_bytes)) return rc;
    DeviceScope restore_device_;
    if (int rc = set_device(device)) return rc;
    return guarded([&]() -> int {
        HostPathCache& hc = host_cache();
        std::lock_guard<std::mutex> lock(hc.mu);
        Backend be(nullptr);
        hc.blob_host = nullptr;
        const size_t need = lce_layout(n, sizeof(idx_t)).total, off_sa = align_up(need), off_lcp = off_sa + align_up(n * sizeof(idx_t));
        host_block(hc, be, device, off_lcp + align_up(n * sizeof(idx_t)) + WS_ALIGN);
        idx_t* dSA = reinterpret_cast<idx_t*>(hc.base + off_sa);
        idx_t* dLCP = reinterpret_cast<idx_t*>(hc.base + off_lcp);
        be.h2d(dSA, SA, n * sizeof(idx_t));
        be.h2d(dLCP, LCP, n * sizeof(idx_t));
        if (int rc = run_lce_build<idx_t>(be, dSA, dLCP, n, hc.base)) return rc;                                  // the caller's blob is not written
        be.d2h(index, hc.base, need);
        be.sync();
        blob_mark_resident(hc, index, need);
        return CAPS_SA_OK;
    });
}

// one batch of queries on a blob at dIndex whose header (hdr, or fetched from the device) is checked first.  mismatches < 0: range_min
// of ranks (A = lo, B = hi), else lce of positions with that many mismatches.  A refused query has 0 in its slot and the call fails.
inline int run_lce_query(Backend& be, const void* dIndex, uint64_t index_bytes, const uint64_t* hdr, const void* dA, const void* dB, uint64_t q,
                         int64_t mismatches, void* dOut)
{
    uint64_t h[LCE_HDR_WORDS];
    if (hdr) std::memcpy(h, hdr, sizeof h);
    else { be.d2h(h, dIndex, sizeof h); be.sync(); }
    LceView v;
    if (int rc = lce_check_header(h, index_bytes, dIndex, v)) return rc;
    if (q == 0) return CAPS_SA_OK;
    uint32_t* flags = reinterpret_cast<uint32_t*>(call_words(be));
    be.memset(flags, 0, sizeof(uint32_t));
    const uint32_t g = capped_grid(std::min<uint64_t>((q + FM_NT - 1) / FM_NT, 1u << 20), FM_NT);
    const uint64_t* A = static_cast<const uint64_t*>(dA);
    const uint64_t* B = static_cast<const uint64_t*>(dB);
    uint64_t* out = static_cast<uint64_t*>(dOut);
    if (mismatches < 0) {
        if (h[LCEH_IDX_BYTES] == 4) CAPS_LAUNCH((lce_range_min_kernel<uint32_t>), g, FM_NT, be, v, A, B, q, out, flags);
        else CAPS_LAUNCH((lce_range_min_kernel<uint64_t>), g, FM_NT, be, v, A, B, q, out, flags);
    } else {
        if (h[LCEH_IDX_BYTES] == 4) CAPS_LAUNCH((lce_query_kernel<uint32_t>), g, FM_NT, be, v, A, B, q, (uint32_t)mismatches, out, flags);
        else CAPS_LAUNCH((lce_query_kernel<uint64_t>), g, FM_NT, be, v, A, B, q, (uint32_t)mismatches, out, flags);
    }
    uint32_t f = 0;
    be.d2h(&f, flags, sizeof f);
    be.sync();
    if (f & 1u) return fail(CAPS_SA_EINVAL, mismatches < 0 ? "a range with lo > hi or hi >= n (its slot holds 0)" : "a position >= n (its slot holds 0)");
    return CAPS_SA_OK;
}
inline int lce_query_device(const void* dIndex, uint64_t index_bytes, const void* dA, const void* dB, uint64_t q, int64_t mismatches, void* dOut,
                            void* stream)
{
    if (int rc = lce_check_blob_args(dIndex, index_bytes)) return rc;
    if (q && (!dA || !dB || !dOut)) return fail(CAPS_SA_EINVAL, "null pointer");
    if (mismatches > (int64_t)LCE_MAX_MISMATCHES) return fail(CAPS_SA_EINVAL, "mismatches must be 0 .. 1024");
    return guarded([&]() -> int {
        Backend be(static_cast<decltype(Backend::stream)>(stream));
        return run_lce_query(be, dIndex, index_bytes, nullptr, dA, dB, q, mismatches, dOut);
    });
}
// the host form: the blob at the head of the host-path block (uploaded unless it is the one there already), the query arrays behind it
inline int lce_query_host(const void* index, uint64_t index_bytes, const uint64_t* A, const uint64_t* B, uint64_t q, int64_t mismatches, uint64_t* out,
                          int device)
{
    if (int rc = lce_check_blob_args(index, index_bytes)) return rc;
    if (q && (!A || !B || !out)) return fail(CAPS_SA_EINVAL, "null pointer");
    if (mismatches > (int64_t)LCE_MAX_MISMATCHES) return fail(CAPS_SA_EINVAL, "mismatches must be 0 .. 1024");
    uint64_t h[LCE_HDR_WORDS];
    std::memcpy(h, index, sizeof h);
    LceView v;
    if (int rc = lce_check_header(h, index_bytes, index, v)) return rc;
    if (q == 0) return CAPS_SA_OK;
    DeviceScope restore_device_;
    if (int rc = set_device(device)) return rc;
    return guarded([&]() -> int {
        HostPathCache& hc = host_cache();
        std::lock_guard<std::mutex> lock(hc.mu);
        Backend be(nullptr);
        const uint64_t blob = h[LCEH_TOTAL];
        const size_t off_a = align_up(blob), off_b = off_a + align_up(q * 8), off_out = off_b + align_up(q * 8);
        blob_upload(hc, be, device, index, blob, off_out + align_up(q * 8));
        be.h2d(hc.base + off_a, A, q * 8);
        be.h2d(hc.base + off_b, B, q * 8);
        const int rc = run_lce_query(be, hc.base, blob, h, hc.base + off_a, hc.base + off_b, q, mismatches, hc.base + off_out);
        if (rc != CAPS_SA_OK && rc != CAPS_SA_EINVAL) return rc;
        be.d2h(out, hc.base + off_out, q * 8);                       // (a refused query: the slots are defined, 0 in the refused ones)
        be.sync();
        return rc;
    });
}

// Text on the device for the kernel-level entry points.
struct DevText {
    uint8_t* raw = nullptr;
    uint32_t* P = nullptr;
    int bits = 0;
};

inline DevText upload_text(Backend& be, DevAllocs& da, const char* T, uint64_t n)
{
    DevText t;
    t.raw = da.get<uint8_t>(n ? n : 1);
    t.P = da.get<uint32_t>(text_alloc_words(n ? n : 1));
    uint32_t* present = da.get<uint32_t>(16);
    uint8_t* lut = da.get<uint8_t>(256);
    be.h2d(t.raw, T, n);
    t.bits = prepare_text(be, t.raw, n, t.P, present, lut);
    return t;
}

template <typename idx_t> SegBufs one_segment(Backend& be, DevAllocs& da, uint64_t cnt)
{
    SegBufs s;
    s.G = 1;
    s.seg_start = da.get<uint64_t>(2);
    s.tile_off = da.get<uint32_t>(2);
    s.tile_rec = da.get<TileInfo>(tiles_of(cnt) + 2);
    s.out2 = da.get<uint64_t>(2);
    CAPS_LAUNCH(uniform_segments_kernel, 1, 256, be, s.seg_start, 1u, cnt, cnt);
    prepare_segments(be, s, tiles_of(cnt));
    return s;
}

template <typename idx_t> ElemBuf<idx_t> elem_buf(DevAllocs& da, uint64_t cnt)
{
    ElemBuf<idx_t> b;
    b.key = da.get<uint64_t>(cnt ? cnt : 1);
    b.sa = da.get<idx_t>(cnt ? cnt : 1);
    b.lcp = da.get<idx_t>(cnt ? cnt : 1);
    return b;
}

template <typename idx_t> int check_positions(const idx_t* v, uint64_t cnt, uint64_t n, const char* what)
{
    for (uint64_t i = 0; i < cnt; ++i)
        if ((uint64_t)v[i] >= n) return fail(CAPS_SA_EINVAL, what);
    return CAPS_SA_OK;
}

template <typename idx_t>
int sort_suffixes(const char* T, uint64_t n, const idx_t* idx, uint64_t cnt, idx_t* out_sa, idx_t* out_lcp, int device)
{
    if (int rc = check_common<idx_t>(T, n, 0)) return rc;
    if (cnt == 0) return CAPS_SA_OK;
    if (!idx || !out_sa || !out_lcp) return fail(CAPS_SA_EINVAL, "null pointer");
    if (int rc = check_positions(idx, cnt, n, "suffix position out of range")) return rc;
    DeviceScope restore_device_;
    if (int rc = set_device(device)) return rc;
    return guarded([&]() -> int {
        Backend be(nullptr);
        DevAllocs da(be);
        DevText t = upload_text(be, da, T, n);
        ElemBuf<idx_t> a = elem_buf<idx_t>(da, cnt), b = elem_buf<idx_t>(da, cnt);
        TileDesc* desc = da.get<TileDesc>(tiles_of(cnt) + 2);
        idx_t* osa = da.get<idx_t>(cnt);
        idx_t* olcp = da.get<idx_t>(cnt);
        be.h2d(a.sa, idx, cnt * sizeof(idx_t));
        SegBufs s = one_segment<idx_t>(be, da, cnt);
        const uint32_t g = (uint32_t)((cnt + 255) / 256);
        if (t.bits == 2) {
            CAPS_LAUNCH((make_keys_kernel<idx_t, 2>), g, 256, be, (const uint32_t*)t.P, (const idx_t*)a.sa, cnt, a.key);
            SortOpts o;
            o.need_lcp = true;
            SortResult<idx_t> r = segmented_sort<idx_t, 2>(be, t.P, n, desc, s, tiles_of(cnt), cnt, a, b, cnt, o);
            finalize<idx_t, 2>(be, t.P, n, r, osa, olcp);
        } else {
            CAPS_LAUNCH((make_keys_kernel<idx_t, 8>), g, 256, be, (const uint32_t*)t.P, (const idx_t*)a.sa, cnt, a.key);
            SortOpts o;
            o.need_lcp = true;
            SortResult<idx_t> r = segmented_sort<idx_t, 8>(be, t.P, n, desc, s, tiles_of(cnt), cnt, a, b, cnt, o);
            finalize<idx_t, 8>(be, t.P, n, r, osa, olcp);
        }
        be.d2h(out_sa, osa, cnt * sizeof(idx_t));
        be.d2h(out_lcp, olcp, cnt * sizeof(idx_t));
        be.sync();
        return CAPS_SA_OK;
    });
}

// Independent sorts of consecutive segments of a suffix list (the shape of phase 2:
// sort_partition over every partition, src/Suffix_Array.cpp:388-404), with finished segments
// sitting out later passes.  out_lcp at a segment head = lcp with the last suffix of the
// previous non-empty segment (what compute_partition_boundary_lcp produces, cpp:431-447).
template <typename idx_t>
int sort_segments(const char* T, uint64_t n, const idx_t* idx, uint64_t cnt, const uint64_t* seg_start, uint64_t G,
                  idx_t* out_sa, idx_t* out_lcp, int device)
{
    if (int rc = check_common<idx_t>(T, n, 0)) return rc;
    if (cnt == 0) return CAPS_SA_OK;
    if (!idx || !out_sa || !out_lcp || !seg_start || G == 0 || G > 0x7fffffffull) return fail(CAPS_SA_EINVAL, "bad argument");
    if (seg_start[0] != 0 || seg_start[G] != cnt) return fail(CAPS_SA_EINVAL, "segments must cover [0, cnt)");
    uint64_t max_len = 0, n_tiles = 0;
    for (uint64_t g = 0; g < G; ++g) {
        if (seg_start[g + 1] < seg_start[g]) return fail(CAPS_SA_EINVAL, "segment offsets must be non-decreasing");
        const uint64_t len = seg_start[g + 1] - seg_start[g];
        max_len = len > max_len ? len : max_len;
        n_tiles += tiles_of(len);
    }
    if (int rc = check_positions(idx, cnt, n, "suffix position out of range")) return rc;
    DeviceScope restore_device_;
    if (int rc = set_device(device)) return rc;
    return guarded([&]() -> int {
        Backend be(nullptr);
        DevAllocs da(be);
        DevText t = upload_text(be, da, T, n);
        ElemBuf<idx_t> a = elem_buf<idx_t>(da, cnt), b = elem_buf<idx_t>(da, cnt);
        TileDesc* desc = da.get<TileDesc>(n_tiles + 2);
        idx_t* osa = da.get<idx_t>(cnt);
        idx_t* olcp = da.get<idx_t>(cnt);
        SegBufs s;
        s.G = (uint32_t)G;
        s.seg_start = da.get<uint64_t>(G + 1);
        s.tile_off = da.get<uint32_t>(G + 1);
        s.tile_rec = da.get<TileInfo>(n_tiles + 2);
        s.out2 = da.get<uint64_t>(2);
        be.h2d(a.sa, idx, cnt * sizeof(idx_t));
        be.h2d(s.seg_start, seg_start, (G + 1) * sizeof(uint64_t));
        prepare_segments(be, s, n_tiles);
        const uint32_t g = (uint32_t)((cnt + 255) / 256);
        if (t.bits == 2) {
            CAPS_LAUNCH((make_keys_kernel<idx_t, 2>), g, 256, be, (const uint32_t*)t.P, (const idx_t*)a.sa, cnt, a.key);
            SortOpts o;
            o.need_lcp = true;
            o.skip_finished = true;
            SortResult<idx_t> r = segmented_sort<idx_t, 2>(be, t.P, n, desc, s, (uint32_t)n_tiles, max_len, a, b, cnt, o);
            finalize<idx_t, 2>(be, t.P, n, r, osa, olcp);
        } else {
            CAPS_LAUNCH((make_keys_kernel<idx_t, 8>), g, 256, be, (const uint32_t*)t.P, (const idx_t*)a.sa, cnt, a.key);
            SortOpts o;
            o.need_lcp = true;
            o.skip_finished = true;
            SortResult<idx_t> r = segmented_sort<idx_t, 8>(be, t.P, n, desc, s, (uint32_t)n_tiles, max_len, a, b, cnt, o);
            finalize<idx_t, 8>(be, t.P, n, r, osa, olcp);
        }
        be.d2h(out_sa, osa, cnt * sizeof(idx_t));
        be.d2h(out_lcp, olcp, cnt * sizeof(idx_t));
        be.sync();
        return CAPS_SA_OK;
    });
}

template <typename idx_t>
int merge_runs(const char* T, uint64_t n, const idx_t* X, uint64_t len_x, const idx_t* Y, uint64_t len_y, const idx_t* LX,
               const idx_t* LY, idx_t* Z, idx_t* LZ, int device)
{
    if (int rc = check_common<idx_t>(T, n, 0)) return rc;
    const uint64_t cnt = len_x + len_y;
    if (cnt == 0) return CAPS_SA_OK;
    if ((len_x && (!X || !LX)) || (len_y && (!Y || !LY)) || !Z || !LZ) return fail(CAPS_SA_EINVAL, "null pointer");
    if (int rc = check_positions(X, len_x, n, "suffix position out of range")) return rc;
    if (int rc = check_positions(Y, len_y, n, "suffix position out of range")) return rc;
    DeviceScope restore_device_;
    if (int rc = set_device(device)) return rc;
    return guarded([&]() -> int {
        Backend be(nullptr);
        DevAllocs da(be);
        DevText t = upload_text(be, da, T, n);
        ElemBuf<idx_t> a = elem_buf<idx_t>(da, cnt), b = elem_buf<idx_t>(da, cnt);
        TileDesc* desc = da.get<TileDesc>(tiles_of(cnt) + 2);
        be.h2d(a.sa, X, len_x * sizeof(idx_t));
        be.h2d(a.sa + len_x, Y, len_y * sizeof(idx_t));
        // LX / LY are accepted for signature parity with the reference's merge; the kernel
        // rebuilds the LCPs of the merged run from the keys (kernels.h, "LCPs").
        (void)LX; (void)LY;
        SegBufs s = one_segment<idx_t>(be, da, cnt);
        const SegDesc sd = s.desc();
        const uint32_t nt = tiles_of(cnt), g = (uint32_t)((cnt + 255) / 256);
        const uint32_t pg = nt < be.persistent_blocks() ? nt : be.persistent_blocks();
        be.memset(desc + nt, 0, sizeof(uint32_t));          // merge_partition_kernel counts the tiles it lists there
        if (t.bits == 2) {
            CAPS_LAUNCH((make_keys_kernel<idx_t, 2>), g, 256, be, (const uint32_t*)t.P, (const idx_t*)a.sa, cnt, a.key);
            CAPS_LAUNCH((merge_partition_kernel<idx_t, 2, true>), (nt + 255) / 256, 256, be, sd, (const uint32_t*)t.P, n, (uint64_t)TILE_E,
                        len_x, 0u, 1u, (const uint64_t*)a.key, (const idx_t*)a.sa, desc, (uint64_t*)nullptr, 0u, reinterpret_cast<uint32_t*>(desc + nt));
            CAPS_LAUNCH((merge_pass_kernel<idx_t, 2, true>), pg, TILE_NT, be, (const TileDesc*)desc, (const uint32_t*)(desc + nt), (const uint32_t*)t.P, n,
                        (const uint64_t*)a.key, (const idx_t*)a.sa, b.key, b.sa, b.lcp, (uint64_t*)nullptr);
        } else {
            CAPS_LAUNCH((make_keys_kernel<idx_t, 8>), g, 256, be, (const uint32_t*)t.P, (const idx_t*)a.sa, cnt, a.key);
            CAPS_LAUNCH((merge_partition_kernel<idx_t, 8, true>), (nt + 255) / 256, 256, be, sd, (const uint32_t*)t.P, n, (uint64_t)TILE_E,
                        len_x, 0u, 1u, (const uint64_t*)a.key, (const idx_t*)a.sa, desc, (uint64_t*)nullptr, 0u, reinterpret_cast<uint32_t*>(desc + nt));
            CAPS_LAUNCH((merge_pass_kernel<idx_t, 8, true>), pg, TILE_NT, be, (const TileDesc*)desc, (const uint32_t*)(desc + nt), (const uint32_t*)t.P, n,
                        (const uint64_t*)a.key, (const idx_t*)a.sa, b.key, b.sa, b.lcp, (uint64_t*)nullptr);
        }
        be.d2h(Z, b.sa, cnt * sizeof(idx_t));
        be.d2h(LZ, b.lcp, cnt * sizeof(idx_t));
        be.sync();
        return CAPS_SA_OK;
    });
}

template <typename idx_t>
int upper_bounds(const char* T, uint64_t n, const idx_t* X, uint64_t cnt, const idx_t* piv, uint64_t npiv, idx_t* out, int device)
{
    if (int rc = check_common<idx_t>(T, n, 0)) return rc;
    if (npiv == 0) return CAPS_SA_OK;
    if ((cnt && !X) || !piv || !out) return fail(CAPS_SA_EINVAL, "null pointer");
    if (npiv > 0x7fffffffull) return fail(CAPS_SA_EINVAL, "too many pivots");
    if (int rc = check_positions(X, cnt, n, "suffix position out of range")) return rc;
    if (int rc = check_positions(piv, npiv, n, "pivot position out of range")) return rc;
    DeviceScope restore_device_;
    if (int rc = set_device(device)) return rc;
    return guarded([&]() -> int {
        Backend be(nullptr);
        DevAllocs da(be);
        DevText t = upload_text(be, da, T, n);
        ElemBuf<idx_t> a = elem_buf<idx_t>(da, cnt), pv = elem_buf<idx_t>(da, npiv);
        idx_t* Pm = da.get<idx_t>(npiv + 2);
        be.h2d(a.sa, X, cnt * sizeof(idx_t));
        be.h2d(pv.sa, piv, npiv * sizeof(idx_t));
        SegBufs s = one_segment<idx_t>(be, da, cnt);
        const uint32_t np = (uint32_t)npiv, bpr = (np + 255) / 256;
        const uint32_t g1 = (uint32_t)((cnt + 255) / 256), g2 = (uint32_t)((npiv + 255) / 256);
        if (t.bits == 2) {
            if (cnt) CAPS_LAUNCH((make_keys_kernel<idx_t, 2>), g1, 256, be, (const uint32_t*)t.P, (const idx_t*)a.sa, cnt, a.key);
            CAPS_LAUNCH((make_keys_kernel<idx_t, 2>), g2, 256, be, (const uint32_t*)t.P, (const idx_t*)pv.sa, npiv, pv.key);
            CAPS_LAUNCH((locate_kernel<idx_t, 2>), bpr, 256, be, (const uint32_t*)t.P, n, (const uint64_t*)s.seg_start, 1u,
                        (const uint64_t*)a.key, (const idx_t*)a.sa, (const uint64_t*)pv.key, (const idx_t*)pv.sa, np, Pm);
        } else {
            if (cnt) CAPS_LAUNCH((make_keys_kernel<idx_t, 8>), g1, 256, be, (const uint32_t*)t.P, (const idx_t*)a.sa, cnt, a.key);
            CAPS_LAUNCH((make_keys_kernel<idx_t, 8>), g2, 256, be, (const uint32_t*)t.P, (const idx_t*)pv.sa, npiv, pv.key);
            CAPS_LAUNCH((locate_kernel<idx_t, 8>), bpr, 256, be, (const uint32_t*)t.P, n, (const uint64_t*)s.seg_start, 1u,
                        (const uint64_t*)a.key, (const idx_t*)a.sa, (const uint64_t*)pv.key, (const idx_t*)pv.sa, np, Pm);
        }
        be.d2h(out, Pm + 1, npiv * sizeof(idx_t));
        be.sync();
        return CAPS_SA_OK;
    });
}

template <typename idx_t>
int lcp_pairs(const char* T, uint64_t n, const idx_t* a, const idx_t* b, uint64_t cnt, idx_t* out, int device)
{
    if (int rc = check_common<idx_t>(T, n, 0)) return rc;
    if (cnt == 0) return CAPS_SA_OK;
    if (!a || !b || !out) return fail(CAPS_SA_EINVAL, "null pointer");
    if (int rc = check_positions(a, cnt, n, "suffix position out of range")) return rc;
    if (int rc = check_positions(b, cnt, n, "suffix position out of range")) return rc;
    DeviceScope restore_device_;
    if (int rc = set_device(device)) return rc;
    return guarded([&]() -> int {
        Backend be(nullptr);
        DevAllocs da(be);
        DevText t = upload_text(be, da, T, n);
        idx_t* da_ = da.get<idx_t>(cnt);
        idx_t* db_ = da.get<idx_t>(cnt);
        idx_t* dout = da.get<idx_t>(cnt);
        be.h2d(da_, a, cnt * sizeof(idx_t));
        be.h2d(db_, b, cnt * sizeof(idx_t));
        const uint32_t g = (uint32_t)((cnt + 255) / 256);
        if (t.bits == 2)
            CAPS_LAUNCH((lcp_pairs_kernel<idx_t, 2>), g, 256, be, (const uint32_t*)t.P, n, (const idx_t*)da_, (const idx_t*)db_, cnt, dout);
        else
            CAPS_LAUNCH((lcp_pairs_kernel<idx_t, 8>), g, 256, be, (const uint32_t*)t.P, n, (const idx_t*)da_, (const idx_t*)db_, cnt, dout);
        be.d2h(out, dout, cnt * sizeof(idx_t));
        be.sync();
        return CAPS_SA_OK;
    });
}

}  // namespace caps

// ---------------------------------------------------------------------------------------
extern "C" {

const char* CAPS_API(last_error)(void) { return caps::last_error_ref().c_str(); }
const char* CAPS_API(version)(void) { return "caps-sa_amd 0.2 (gfx950)"; }
uint32_t CAPS_API(stats_bytes)(void) { return (uint32_t)sizeof(caps_sa_stats); }
uint32_t CAPS_API(shard_info_bytes)(void) { return (uint32_t)sizeof(caps_sa_shard_info); }

void CAPS_API(release_cache)(void)
{
    caps::HostPathCache& hc = caps::host_cache();
    std::lock_guard<std::mutex> lock(hc.mu);
    caps::DeviceScope restore_device_;
    if (hc.device >= 0 && caps::set_device(hc.device) != CAPS_SA_OK) return;
    caps::release_host_cache_locked(hc);
}

int CAPS_API(gen_rand_seq)(uint32_t seed, uint64_t n, char* out_)
{
    if (!out_ && n) return caps::fail(CAPS_SA_EINVAL, "null pointer");
    char* __restrict__ out = out_;
    // MT19937 (Matsumoto & Nishimura): init_genrand(19650218), then init_by_array with the one-word key {seed} -- what
    // CPython's random.seed(int) does for 0 <= seed < 2^32
    constexpr int N = 624, M = 397;
    alignas(64) uint32_t mt[N];
    mt[0] = 19650218u;
    for (int i = 1; i < N; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
    {
        int i = 1;
        for (int k = N; k; --k) {                                   // key length 1: j stays 0
            mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1664525u)) + seed;
            if (++i >= N) { mt[0] = mt[N - 1]; i = 1; }
        }
        for (int k = N - 1; k; --k) {
            mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1566083941u)) - (uint32_t)i;
            if (++i >= N) { mt[0] = mt[N - 1]; i = 1; }
        }
        mt[0] = 0x80000000u;
    }
    // a block of 624 outputs at a time: the recurrence in three loops without wrap-around (the first two vectorise: their
    // dependence distance is 227), tempering into a buffer, then a branch-free compaction of the accepted draws
    auto twist = [](uint32_t a, uint32_t b, uint32_t c) {
        const uint32_t y = (a & 0x80000000u) | (b & 0x7FFFFFFFu);
        return c ^ (y >> 1) ^ ((0u - (y & 1u)) & 0x9908B0DFu);
    };
    alignas(64) uint8_t k3[N + 8];
    char tail[N + 8];
    uint64_t done = 0;
    while (done < n) {
        for (int k = 0; k < N - M; ++k) mt[k] = twist(mt[k], mt[k + 1], mt[k + M]);
        for (int k = N - M; k < N - 1; ++k) mt[k] = twist(mt[k], mt[k + 1], mt[k + M - N]);
        mt[N - 1] = twist(mt[N - 1], mt[0], mt[M - 1]);
        for (int k = 0; k < N; ++k) {
            uint32_t y = mt[k];
            y ^= y >> 11;
            y ^= (y << 7) & 0x9D2C5680u;
            y ^= (y << 15) & 0xEFC60000u;
            y ^= y >> 18;
            k3[k] = (uint8_t)(y >> 29);                             // getrandbits(3); a draw >= 4 is rejected
        }
        char* __restrict__ o = n - done >= (uint64_t)N ? out + done : tail;      // room for a whole block: straight into the output
        uint32_t c = 0;
        for (int k = 0; k < N; ++k) { const uint8_t v = k3[k]; o[c] = "ACGTACGT"[v]; c += v < 4 ? 1u : 0u; }
        if (o == tail) { if (c > n - done) c = (uint32_t)(n - done); std::memcpy(out + done, tail, c); }
        done += c;
    }
    return CAPS_SA_OK;
}

void* CAPS_API(host_alloc)(uint64_t bytes)
{
    void* p = nullptr;
    caps::guarded([&]() -> int { p = caps::Backend::host_alloc(bytes); return CAPS_SA_OK; });
    return p;
}

void CAPS_API(host_free)(void* p) { caps::Backend::host_free(p); }

int CAPS_API(workspace_bytes_ex)(uint64_t n, uint64_t subproblem_count, int idx_bytes, int bits_per_char, uint64_t* bytes)
{
    if (!bytes || (idx_bytes != 4 && idx_bytes != 8) || (bits_per_char != 2 && bits_per_char != 8)) return caps::fail(CAPS_SA_EINVAL, "bad argument");
    *bytes = caps::ws_reported(idx_bytes == 4 ? caps::make_plan<uint32_t>(n, subproblem_count, nullptr, bits_per_char).bytes
                                              : caps::make_plan<uint64_t>(n, subproblem_count, nullptr, bits_per_char).bytes);
    return CAPS_SA_OK;
}
int CAPS_API(workspace_bytes)(uint64_t n, uint64_t subproblem_count, int idx_bytes, uint64_t* bytes)
{
    return CAPS_API(workspace_bytes_ex)(n, subproblem_count, idx_bytes, 8, bytes);
}

#define CAPS_DEFINE_WIDTH(SFX, IDX)                                                                                        \
    int CAPS_API(build_##SFX)(const char* T, uint64_t n, uint64_t p, uint64_t ctx, IDX* SA, IDX* LCP, int device,          \
                              caps_sa_stats* st)                                                                           \
    { return caps::build_host<IDX>(T, n, p, ctx, SA, LCP, device, st); }                                                   \
    int CAPS_API(build_multi_##SFX)(const char* T, uint64_t n, uint64_t p, uint64_t ctx, IDX* SA, IDX* LCP,                \
                                    const int* devices, int n_devices, caps_sa_stats* st)                                  \
    { return caps::build_multi<IDX>(T, n, p, ctx, SA, LCP, devices, n_devices, st); }                                      \
    int CAPS_API(build_device_##SFX)(const void* dT, uint64_t n, uint64_t p, uint64_t ctx, void* dSA, void* dLCP,          \
                                     void* ws, uint64_t ws_bytes, void* stream, caps_sa_stats* st)                         \
    { return caps::build_device<IDX>(dT, n, p, ctx, dSA, dLCP, ws, ws_bytes, stream, st); }                                \
    int CAPS_API(build_bwt_##SFX)(const char* T, uint64_t n, uint64_t p, uint64_t ctx, IDX* SA, IDX* LCP, uint8_t* BWT,       \
                                  uint64_t* primary, int device, caps_sa_stats* st)                                        \
    { return caps::build_bwt<IDX>(T, n, p, ctx, SA, LCP, BWT, primary, device, st); }                                      \
    int CAPS_API(bwt_device_##SFX)(const void* dT, uint64_t n, const void* dSA, uint64_t first, uint64_t cnt, void* dBWT,   \
                                   void* stream, uint64_t* primary)                                                        \
    { return caps::bwt_device<IDX>(dT, n, dSA, first, cnt, dBWT, stream, primary); }                                       \
    int CAPS_API(verify_device_##SFX)(const void* dT, uint64_t n, const void* dSA, const void* dLCP, void* stream,          \
                                      uint64_t* n_errors)                                                                  \
    { return caps::verify_device<IDX>(dT, n, dSA, dLCP, stream, n_errors, n, 1u); }                                        \
    int CAPS_API(verify_slice_device_##SFX)(const void* dT, uint64_t n, const void* dSA, const void* dLCP, uint64_t cnt,    \
                                            int is_head, void* stream, uint64_t* n_errors)                                 \
    { return caps::verify_device<IDX>(dT, n, dSA, dLCP, stream, n_errors, cnt, is_head ? 1u : 0u); }                       \
    int CAPS_API(sort_suffixes_##SFX)(const char* T, uint64_t n, const IDX* idx, uint64_t cnt, IDX* osa, IDX* olcp, int d) \
    { return caps::sort_suffixes<IDX>(T, n, idx, cnt, osa, olcp, d); }                                                     \
    int CAPS_API(sort_segments_##SFX)(const char* T, uint64_t n, const IDX* idx, uint64_t cnt, const uint64_t* seg,        \
                                      uint64_t G, IDX* osa, IDX* olcp, int d)                                              \
    { return caps::sort_segments<IDX>(T, n, idx, cnt, seg, G, osa, olcp, d); }                                             \
    int CAPS_API(merge_##SFX)(const char* T, uint64_t n, const IDX* X, uint64_t lx, const IDX* Y, uint64_t ly,             \
                              const IDX* LX, const IDX* LY, IDX* Z, IDX* LZ, int d)                                        \
    { return caps::merge_runs<IDX>(T, n, X, lx, Y, ly, LX, LY, Z, LZ, d); }                                                \
    int CAPS_API(upper_bound_##SFX)(const char* T, uint64_t n, const IDX* X, uint64_t cnt, const IDX* piv, uint64_t np,    \
                                    IDX* out, int d)                                                                       \
    { return caps::upper_bounds<IDX>(T, n, X, cnt, piv, np, out, d); }                                                     \
    int CAPS_API(lcp_##SFX)(const char* T, uint64_t n, const IDX* a, const IDX* b, uint64_t cnt, IDX* out, int d)          \
    { return caps::lcp_pairs<IDX>(T, n, a, b, cnt, out, d); }

CAPS_DEFINE_WIDTH(u32, uint32_t)
CAPS_DEFINE_WIDTH(u64, uint64_t)

int CAPS_API(inverse_bwt_workspace_bytes)(uint64_t n, int idx_bytes, uint64_t* bytes) { return caps::inverse_bwt_workspace_bytes(n, idx_bytes, bytes); }
#define CAPS_DEFINE_INVERSE(SFX, IDX)                                                                                      \
    int CAPS_API(inverse_bwt_device_##SFX)(const void* dBWT, uint64_t n, uint64_t primary, void* dT, void* ws,             \
                                           uint64_t ws_bytes, void* stream)                                                \
    { return caps::inverse_bwt_device<IDX>(dBWT, n, primary, dT, ws, ws_bytes, stream); }                                  \
    int CAPS_API(inverse_bwt_##SFX)(const uint8_t* BWT, uint64_t n, uint64_t primary, char* T, int device)                 \
    { return caps::inverse_bwt_host<IDX>(BWT, n, primary, T, device); }
CAPS_DEFINE_INVERSE(u32, uint32_t)
CAPS_DEFINE_INVERSE(u64, uint64_t)

int CAPS_API(fm_index_bytes)(uint64_t n, uint32_t sa_sample, int idx_bytes, uint64_t* bytes) { return caps::fm_index_bytes(n, sa_sample, idx_bytes, bytes); }
#define CAPS_DEFINE_FM(SFX, IDX)                                                                                           \
    int CAPS_API(fm_build_device_##SFX)(const void* dBWT, uint64_t n, uint64_t primary, const void* dSA, uint32_t sa_sample, \
                                        void* dIndex, uint64_t index_bytes, void* stream)                                  \
    { return caps::fm_build_device<IDX>(dBWT, n, primary, dSA, sa_sample, dIndex, index_bytes, stream); }                  \
    int CAPS_API(fm_build_##SFX)(const uint8_t* BWT, uint64_t n, uint64_t primary, const IDX* SA, uint32_t sa_sample,      \
                                 void* index, uint64_t index_bytes, int device)                                            \
    { return caps::fm_build_host<IDX>(BWT, n, primary, SA, sa_sample, index, index_bytes, device); }
CAPS_DEFINE_FM(u32, uint32_t)
CAPS_DEFINE_FM(u64, uint64_t)
int CAPS_API(fm_wide_index_bytes)(uint64_t n, uint32_t sigma, uint32_t sa_sample, int idx_bytes, uint64_t* bytes)
{ return caps::fmw_index_bytes(n, sigma, sa_sample, idx_bytes, bytes); }
int CAPS_API(fm_wide_workspace_bytes)(uint64_t n, int idx_bytes, uint64_t* bytes) { return caps::fmw_workspace_bytes(n, idx_bytes, bytes); }
#define CAPS_DEFINE_FM_WIDE(SFX, IDX)                                                                                                \
    int CAPS_API(fm_build_wide_device_##SFX)(const void* dBWT, uint64_t n, uint64_t primary, const void* dSA, uint32_t sa_sample,   \
                                             void* dIndex, uint64_t index_capacity, void* workspace, uint64_t workspace_bytes, void* stream) \
    { return caps::fmw_build_device<IDX>(dBWT, n, primary, dSA, sa_sample, dIndex, index_capacity, workspace, workspace_bytes, stream); } \
    int CAPS_API(fm_build_wide_##SFX)(const uint8_t* BWT, uint64_t n, uint64_t primary, const IDX* SA, uint32_t sa_sample,          \
                                      void* index, uint64_t index_capacity, int device)                                             \
    { return caps::fmw_build_host<IDX>(BWT, n, primary, SA, sa_sample, index, index_capacity, device); }
CAPS_DEFINE_FM_WIDE(u32, uint32_t)
CAPS_DEFINE_FM_WIDE(u64, uint64_t)
#undef CAPS_DEFINE_FM_WIDE
int CAPS_API(fm_from_bwt_workspace_bytes)(uint64_t n, uint32_t sa_sample, int idx_bytes, uint64_t* bytes)
{ return caps::fm_from_bwt_workspace_bytes(n, sa_sample, idx_bytes, bytes); }
#define CAPS_FM_FROM_BWT(SFX, IDX)                                                                                                  \
    int CAPS_API(fm_build_from_bwt_device_##SFX)(const void* dBWT, uint64_t n, uint64_t primary, uint32_t sa_sample, void* dIndex,  \
                                                 uint64_t index_bytes, void* workspace, uint64_t workspace_bytes, void* stream)     \
    { return caps::fm_build_from_bwt_device<IDX>(dBWT, n, primary, sa_sample, dIndex, index_bytes, workspace, workspace_bytes, stream); } \
    int CAPS_API(fm_build_from_bwt_##SFX)(const uint8_t* BWT, uint64_t n, uint64_t primary, uint32_t sa_sample, void* index,        \
                                          uint64_t index_bytes, int device)                                                        \
    { return caps::fm_build_from_bwt_host<IDX>(BWT, n, primary, sa_sample, index, index_bytes, device); }
CAPS_FM_FROM_BWT(u32, uint32_t)
CAPS_FM_FROM_BWT(u64, uint64_t)
#undef CAPS_FM_FROM_BWT
int CAPS_API(fm_index_bytes_ex)(uint64_t n, uint32_t sa_sample, uint32_t text_sample, int idx_bytes, uint64_t* bytes)
{ return caps::fm_index_bytes_ex(n, sa_sample, text_sample, idx_bytes, bytes); }
int CAPS_API(fm_add_text_samples_device)(void* dIndex, uint64_t index_bytes, uint32_t text_sample, void* stream)
{ return caps::fm_add_text_samples_device(dIndex, index_bytes, text_sample, stream); }
int CAPS_API(fm_add_text_samples)(void* index, uint64_t index_bytes, uint32_t text_sample, int device)
{ return caps::fm_add_text_samples_host(index, index_bytes, text_sample, device); }
int CAPS_API(fm_extract_workspace_bytes)(uint64_t q, uint64_t* bytes) { return caps::fm_extract_workspace_bytes(q, bytes); }
int CAPS_API(fm_extract_device)(const void* dIndex, uint64_t index_bytes, const void* dStart, const void* dOutOff, uint64_t q, void* dText,
                                void* workspace, uint64_t workspace_bytes, void* stream)
{ return caps::fm_extract_device(dIndex, index_bytes, dStart, dOutOff, q, dText, workspace, workspace_bytes, stream); }
int CAPS_API(fm_extract)(const void* index, uint64_t index_bytes, const uint64_t* start, const uint64_t* out_off, uint64_t q, uint8_t* text,
                         int device)
{ return caps::fm_extract_host(index, index_bytes, start, out_off, q, text, device); }
int CAPS_API(fm_count_device)(const void* dIndex, uint64_t index_bytes, const void* dPatterns, const void* dPatOff, uint64_t q,
                              void* dFirst, void* dCount, void* stream)
{ return caps::fm_count_device(dIndex, index_bytes, dPatterns, dPatOff, q, dFirst, dCount, stream); }
int CAPS_API(fm_locate_device)(const void* dIndex, uint64_t index_bytes, const void* dFirst, const void* dCount, const void* dOutOff,
                               uint64_t q, void* dPos, void* stream)
{ return caps::fm_locate_device(dIndex, index_bytes, dFirst, dCount, dOutOff, q, dPos, stream); }
int CAPS_API(fm_count)(const void* index, uint64_t index_bytes, const uint8_t* patterns, const uint64_t* pat_off, uint64_t q,
                       uint64_t* first, uint64_t* count, int device)
{ return caps::fm_count_host(index, index_bytes, patterns, pat_off, q, first, count, device); }
int CAPS_API(fm_locate)(const void* index, uint64_t index_bytes, const uint64_t* first, const uint64_t* count, const uint64_t* out_off,
                        uint64_t q, uint64_t* pos, int device)
{ return caps::fm_locate_host(index, index_bytes, first, count, out_off, q, pos, device); }
int CAPS_API(fm_match_device)(const void* dIndex, uint64_t index_bytes, const void* dPatterns, const void* dPatOff, uint64_t q, uint32_t max_len,
                              void* dLen, void* dFirst, void* dCount, void* stream)
{ return caps::fm_match_device(dIndex, index_bytes, dPatterns, dPatOff, q, max_len, dLen, dFirst, dCount, stream); }
int CAPS_API(fm_match)(const void* index, uint64_t index_bytes, const uint8_t* patterns, const uint64_t* pat_off, uint64_t q, uint32_t max_len,
                       uint32_t* len, uint64_t* first, uint64_t* count, int device)
{ return caps::fm_match_host(index, index_bytes, patterns, pat_off, q, max_len, len, first, count, device); }
int CAPS_API(kmer_workspace_bytes)(uint64_t n, int idx_bytes, uint64_t* bytes) { return caps::kmer_workspace_bytes(n, idx_bytes, bytes); }
#define CAPS_DEFINE_KMER(SFX, IDX)                                                                                          \
    int CAPS_API(kmers_device_##SFX)(const void* dSA, const void* dLCP, uint64_t n, uint64_t k, uint64_t min_count,         \
                                     uint64_t max_count, void* dRecords, uint64_t capacity, uint64_t* n_records, void* ws,  \
                                     uint64_t ws_bytes, void* stream)                                                       \
    { return caps::kmers_device<IDX>(dSA, dLCP, n, k, min_count, max_count, dRecords, capacity, n_records, ws, ws_bytes, stream); } \
    int CAPS_API(kmer_spectrum_device_##SFX)(const void* dSA, const void* dLCP, uint64_t n, uint64_t k, uint32_t bins,      \
                                             uint64_t* hist, void* ws, uint64_t ws_bytes, void* stream)                     \
    { return caps::kmer_spectrum_device<IDX>(dSA, dLCP, n, k, bins, hist, ws, ws_bytes, stream); }                          \
    int CAPS_API(kmer_census_device_##SFX)(const void* dSA, const void* dLCP, uint64_t n, uint32_t max_k, uint64_t* distinct, \
                                           uint64_t* unique, void* ws, uint64_t ws_bytes, void* stream)                     \
    { return caps::kmer_census_device<IDX>(dSA, dLCP, n, max_k, distinct, unique, ws, ws_bytes, stream); }                  \
    int CAPS_API(kmers_##SFX)(const IDX* SA, const IDX* LCP, uint64_t n, uint64_t k, uint64_t min_count, uint64_t max_count, \
                              void* records, uint64_t capacity, uint64_t* n_records, int device)                            \
    { return caps::kmers_host<IDX>(SA, LCP, n, k, min_count, max_count, records, capacity, n_records, device); }            \
    int CAPS_API(kmer_spectrum_##SFX)(const IDX* SA, const IDX* LCP, uint64_t n, uint64_t k, uint32_t bins, uint64_t* hist, \
                                      int device)                                                                           \
    { return caps::kmer_spectrum_host<IDX>(SA, LCP, n, k, bins, hist, device); }                                            \
    int CAPS_API(kmer_census_##SFX)(const IDX* SA, const IDX* LCP, uint64_t n, uint32_t max_k, uint64_t* distinct,          \
                                    uint64_t* unique, int device)                                                           \
    { return caps::kmer_census_host<IDX>(SA, LCP, n, max_k, distinct, unique, device); }
CAPS_DEFINE_KMER(u32, uint32_t)
CAPS_DEFINE_KMER(u64, uint64_t)
#undef CAPS_DEFINE_KMER
int CAPS_API(cross_workspace_bytes)(uint64_t n, int idx_bytes, uint64_t* bytes) { return caps::cross_workspace_bytes(n, idx_bytes, bytes); }
#define CAPS_DEFINE_CROSS(SFX, IDX)                                                                                         \
    int CAPS_API(cross_mums_device_##SFX)(const void* dSA, const void* dLCP, const void* dBWT, uint64_t n, uint64_t split,  \
                                          uint64_t min_len, void* dRecords, uint64_t capacity, uint64_t* summary, void* ws, \
                                          uint64_t ws_bytes, void* stream)                                                  \
    { return caps::cross_device<IDX>(dSA, dLCP, dBWT, n, split, min_len, false, 0, dRecords, capacity, summary, ws, ws_bytes, stream); } \
    int CAPS_API(cross_mems_device_##SFX)(const void* dSA, const void* dLCP, const void* dBWT, uint64_t n, uint64_t split,  \
                                          uint64_t min_len, uint32_t max_occ, void* dRecords, uint64_t capacity,            \
                                          uint64_t* summary, void* ws, uint64_t ws_bytes, void* stream)                     \
    { return caps::cross_device<IDX>(dSA, dLCP, dBWT, n, split, min_len, true, max_occ, dRecords, capacity, summary, ws, ws_bytes, stream); } \
    int CAPS_API(cross_mums_##SFX)(const IDX* SA, const IDX* LCP, const uint8_t* BWT, uint64_t n, uint64_t split,           \
                                   uint64_t min_len, void* records, uint64_t capacity, uint64_t* summary, int device)       \
    { return caps::cross_host<IDX>(SA, LCP, BWT, n, split, min_len, false, 0, records, capacity, summary, device); }        \
    int CAPS_API(cross_mems_##SFX)(const IDX* SA, const IDX* LCP, const uint8_t* BWT, uint64_t n, uint64_t split,           \
                                   uint64_t min_len, uint32_t max_occ, void* records, uint64_t capacity, uint64_t* summary, \
                                   int device)                                                                              \
    { return caps::cross_host<IDX>(SA, LCP, BWT, n, split, min_len, true, max_occ, records, capacity, summary, device); }
CAPS_DEFINE_CROSS(u32, uint32_t)
CAPS_DEFINE_CROSS(u64, uint64_t)
#undef CAPS_DEFINE_CROSS
int CAPS_API(coll_workspace_bytes)(uint64_t n, int idx_bytes, uint64_t* bytes) { return caps::coll_workspace_bytes(n, idx_bytes, bytes); }
#define CAPS_DEFINE_COLL(SFX, IDX)                                                                                          \
    int CAPS_API(coll_kmers_device_##SFX)(const void* dSA, const void* dLCP, uint64_t n, uint64_t k, const uint64_t* doc_start, \
                                          const uint64_t* doc_len, uint32_t m, uint64_t min_docs, uint64_t max_docs,        \
                                          uint64_t all_of, uint64_t none_of, void* dRecords, uint64_t capacity,             \
                                          uint64_t* n_records, void* ws, uint64_t ws_bytes, void* stream)                   \
    { return caps::coll_kmers_device<IDX>(dSA, dLCP, n, k, caps::CollDocs{doc_start, doc_len, m},                           \
                                          caps::CkFilter{min_docs, max_docs, all_of, none_of}, dRecords, capacity, n_records, ws, ws_bytes, stream); } \
    int CAPS_API(coll_sharing_device_##SFX)(const void* dSA, const void* dLCP, uint64_t n, uint64_t k, const uint64_t* doc_start, \
                                            const uint64_t* doc_len, uint32_t m, uint64_t* freq, uint64_t* shared, void* ws, \
                                            uint64_t ws_bytes, void* stream)                                                \
    { return caps::coll_sharing_device<IDX>(dSA, dLCP, n, k, caps::CollDocs{doc_start, doc_len, m}, freq, shared, ws, ws_bytes, stream); } \
    int CAPS_API(coll_kmers_##SFX)(const IDX* SA, const IDX* LCP, uint64_t n, uint64_t k, const uint64_t* doc_start,        \
                                   const uint64_t* doc_len, uint32_t m, uint64_t min_docs, uint64_t max_docs, uint64_t all_of, \
                                   uint64_t none_of, void* records, uint64_t capacity, uint64_t* n_records, int device)     \
    { return caps::coll_kmers_host<IDX>(SA, LCP, n, k, caps::CollDocs{doc_start, doc_len, m},                               \
                                        caps::CkFilter{min_docs, max_docs, all_of, none_of}, records, capacity, n_records, device); } \
    int CAPS_API(coll_sharing_##SFX)(const IDX* SA, const IDX* LCP, uint64_t n, uint64_t k, const uint64_t* doc_start,      \
                                     const uint64_t* doc_len, uint32_t m, uint64_t* freq, uint64_t* shared, int device)     \
    { return caps::coll_sharing_host<IDX>(SA, LCP, n, k, caps::CollDocs{doc_start, doc_len, m}, freq, shared, device); }
CAPS_DEFINE_COLL(u32, uint32_t)
CAPS_DEFINE_COLL(u64, uint64_t)
#undef CAPS_DEFINE_COLL
int CAPS_API(lpf_workspace_bytes)(uint64_t n, int idx_bytes, uint64_t* bytes) { return caps::lpf_workspace_bytes(n, idx_bytes, bytes); }
int CAPS_API(lz77_workspace_bytes)(uint64_t n, int idx_bytes, uint64_t* bytes) { return caps::lz77_workspace_bytes(n, idx_bytes, bytes); }
#define CAPS_DEFINE_LZ(SFX, IDX)                                                                                            \
    int CAPS_API(lpf_device_##SFX)(const void* dSA, const void* dLCP, uint64_t n, void* dLPF, void* dPrev, void* ws,        \
                                   uint64_t ws_bytes, void* stream)                                                         \
    { return caps::lpf_device<IDX>(dSA, dLCP, n, dLPF, dPrev, ws, ws_bytes, stream); }                                      \
    int CAPS_API(lpf_##SFX)(const IDX* SA, const IDX* LCP, uint64_t n, IDX* LPF, IDX* Prev, int device)                     \
    { return caps::lpf_host<IDX>(SA, LCP, n, LPF, Prev, device); }                                                          \
    int CAPS_API(lz77_device_##SFX)(const void* dLPF, const void* dPrev, uint64_t n, void* dRecords, uint64_t capacity,     \
                                    uint64_t* n_phrases, void* ws, uint64_t ws_bytes, void* stream)                         \
    { return caps::lz77_device<IDX>(dLPF, dPrev, n, dRecords, capacity, n_phrases, ws, ws_bytes, stream); }                 \
    int CAPS_API(lz77_##SFX)(const IDX* SA, const IDX* LCP, uint64_t n, void* records, uint64_t capacity,                   \
                             uint64_t* n_phrases, int device)                                                               \
    { return caps::lz77_host<IDX>(SA, LCP, n, records, capacity, n_phrases, device); }
CAPS_DEFINE_LZ(u32, uint32_t)
CAPS_DEFINE_LZ(u64, uint64_t)
#undef CAPS_DEFINE_LZ
int CAPS_API(lce_index_bytes)(uint64_t n, int idx_bytes, uint64_t* bytes) { return caps::lce_index_bytes(n, idx_bytes, bytes); }
#define CAPS_DEFINE_LCE(SFX, IDX)                                                                                           \
    int CAPS_API(isa_device_##SFX)(const void* dSA, uint64_t n, void* dISA, void* stream)                                   \
    { return caps::isa_device<IDX>(dSA, n, dISA, stream); }                                                                 \
    int CAPS_API(isa_##SFX)(const IDX* SA, uint64_t n, IDX* ISA, int device) { return caps::isa_host<IDX>(SA, n, ISA, device); } \
    int CAPS_API(lce_build_device_##SFX)(const void* dSA, const void* dLCP, uint64_t n, void* dIndex, uint64_t index_bytes, \
                                         void* stream)                                                                      \
    { return caps::lce_build_device<IDX>(dSA, dLCP, n, dIndex, index_bytes, stream); }                                      \
    int CAPS_API(lce_build_##SFX)(const IDX* SA, const IDX* LCP, uint64_t n, void* index, uint64_t index_bytes, int device) \
    { return caps::lce_build_host<IDX>(SA, LCP, n, index, index_bytes, device); }
CAPS_DEFINE_LCE(u32, uint32_t)
CAPS_DEFINE_LCE(u64, uint64_t)
#undef CAPS_DEFINE_LCE
int CAPS_API(lce_range_min_device)(const void* dIndex, uint64_t index_bytes, const void* dLo, const void* dHi, uint64_t q, void* dMin, void* stream)
{ return caps::lce_query_device(dIndex, index_bytes, dLo, dHi, q, -1, dMin, stream); }
int CAPS_API(lce_range_min)(const void* index, uint64_t index_bytes, const uint64_t* lo, const uint64_t* hi, uint64_t q, uint64_t* min, int device)
{ return caps::lce_query_host(index, index_bytes, lo, hi, q, -1, min, device); }
int CAPS_API(lce_device)(const void* dIndex, uint64_t index_bytes, const void* dI, const void* dJ, uint64_t q, uint64_t mismatches, void* dLen,
                         void* stream)
{ return caps::lce_query_device(dIndex, index_bytes, dI, dJ, q, (int64_t)std::min<uint64_t>(mismatches, 1025), dLen, stream); }
int CAPS_API(lce)(const void* index, uint64_t index_bytes, const uint64_t* i, const uint64_t* j, uint64_t q, uint64_t mismatches, uint64_t* len,
                  int device)
{ return caps::lce_query_host(index, index_bytes, i, j, q, (int64_t)std::min<uint64_t>(mismatches, 1025), len, device); }

int CAPS_API(fm_mems_workspace_bytes)(uint64_t total_pattern_bytes, uint64_t q, uint64_t* bytes)
{ return caps::fm_mems_workspace_bytes(total_pattern_bytes, q, bytes); }
int CAPS_API(fm_mems_device)(const void* dIndex, uint64_t index_bytes, const void* dPatterns, const void* dPatOff, uint64_t q, uint32_t min_len,
                             void* dMemOff, void* dMems, uint64_t mem_capacity, void* workspace, uint64_t workspace_bytes, void* stream)
{ return caps::fm_mems_device(dIndex, index_bytes, dPatterns, dPatOff, q, min_len, dMemOff, dMems, mem_capacity, workspace, workspace_bytes, stream); }
int CAPS_API(fm_mems)(const void* index, uint64_t index_bytes, const uint8_t* patterns, const uint64_t* pat_off, uint64_t q, uint32_t min_len,
                      uint64_t* mem_off, void* mems, uint64_t mem_capacity, int device)
{ return caps::fm_mems_host(index, index_bytes, patterns, pat_off, q, min_len, mem_off, mems, mem_capacity, device); }


struct caps_sa_shard { std::unique_ptr<caps::ShardBase> impl; };

caps_sa_shard* caps_shard_new(const void* dT, uint64_t n, uint64_t p, int idx_bytes, int rank, int world, void* stream)
{
    caps_sa_shard* s = new caps_sa_shard;
    try {
        if (idx_bytes == 4) s->impl.reset(new caps::Shard<uint32_t>(dT, n, p, rank, world, stream));
        else s->impl.reset(new caps::Shard<uint64_t>(dT, n, p, rank, world, stream));
    } catch (...) { delete s; throw; }
    return s;
}

int CAPS_API(shard_create)(const void* dT, uint64_t n, uint64_t p, int idx_bytes, int rank, int world, void* stream,
                           caps_sa_shard** out)
{
    if (!out || !dT || (idx_bytes != 4 && idx_bytes != 8) || world < 1 || rank < 0 || rank >= world)
        return caps::fail(CAPS_SA_EINVAL, "bad argument");
    if (idx_bytes == 4 && n > 0xFFFFFFFFull) return caps::fail(CAPS_SA_EINVAL, "n does not fit 32-bit indices");
    *out = nullptr;
    return caps::guarded([&]() -> int { *out = caps_shard_new(dT, n, p, idx_bytes, rank, world, stream); return CAPS_SA_OK; });
}
void CAPS_API(shard_destroy)(caps_sa_shard* s) { delete s; }
int CAPS_API(shard_info)(const caps_sa_shard* s, caps_sa_shard_info* info)
{
    if (!s || !info) return caps::fail(CAPS_SA_EINVAL, "null pointer");
    s->impl->info(info);
    return CAPS_SA_OK;
}
int CAPS_API(shard_phase1)(caps_sa_shard* s, void* k, void* a)
{
    if (!s) return caps::fail(CAPS_SA_EINVAL, "null shard");
    return caps::guarded([&]() -> int { s->impl->phase1(k, a); return CAPS_SA_OK; });
}
int CAPS_API(shard_pivots)(caps_sa_shard* s, const void* k, const void* a, void* sizes)
{
    if (!s || !k || !a || !sizes) return caps::fail(CAPS_SA_EINVAL, "null pointer");
    return caps::guarded([&]() -> int { s->impl->pivots(k, a, sizes); return CAPS_SA_OK; });
}
int CAPS_API(shard_collate)(caps_sa_shard* s, const uint64_t* all_sizes, void* k, void* a, uint64_t* sc, uint64_t* rc)
{
    if (!s || !all_sizes || !sc || !rc) return caps::fail(CAPS_SA_EINVAL, "null pointer");
    return caps::guarded([&]() -> int { s->impl->collate(all_sizes, k, a, sc, rc); return CAPS_SA_OK; });
}
int CAPS_API(shard_phase2)(caps_sa_shard* s, const void* k, const void* a, void* dSA, void* dLCP)
{
    if (!s) return caps::fail(CAPS_SA_EINVAL, "null shard");
    return caps::guarded([&]() -> int { s->impl->phase2(k, a, dSA, dLCP); return CAPS_SA_OK; });
}
int CAPS_API(shard_scatter)(caps_sa_shard* s, void* k, void* a, void* report)
{
    if (!s || !k || !a || !report) return caps::fail(CAPS_SA_EINVAL, "null pointer");
    return caps::guarded([&]() -> int { s->impl->scatter(k, a, report); return CAPS_SA_OK; });
}
int CAPS_API(shard_plan)(caps_sa_shard* s, const uint64_t* all_reports, uint64_t* sc, uint64_t* rc)
{
    if (!s || !all_reports || !sc || !rc) return caps::fail(CAPS_SA_EINVAL, "null pointer");
    return caps::guarded([&]() -> int { return s->impl->plan(all_reports, sc, rc); });
}
int CAPS_API(shard_sort)(caps_sa_shard* s, const void* k, const void* a, void* dSA, void* dLCP)
{
    if (!s) return caps::fail(CAPS_SA_EINVAL, "null shard");
    return caps::guarded([&]() -> int { return s->impl->sort_owned(k, a, dSA, dLCP); });
}
int CAPS_API(shard_set_key_bits)(caps_sa_shard* s, int bits)
{
    if (!s || (bits != 32 && bits != 64)) return caps::fail(CAPS_SA_EINVAL, "bad argument");
    s->impl->set_key_bits(bits);
    return CAPS_SA_OK;
}
int CAPS_API(shard_phase1_arrays)(caps_sa_shard* s, void* d_keys_out, void* d_sa_out, uint64_t* count, uint64_t* subarray_len)
{
    if (!s || !count || !subarray_len) return caps::fail(CAPS_SA_EINVAL, "null pointer");
    return caps::guarded([&]() -> int { s->impl->phase1_arrays(d_keys_out, d_sa_out, count, subarray_len); return CAPS_SA_OK; });
}
int CAPS_API(shard_last_sa)(caps_sa_shard* s, uint64_t* last_sa)
{
    if (!s || !last_sa) return caps::fail(CAPS_SA_EINVAL, "null pointer");
    return caps::guarded([&]() -> int { *last_sa = s->impl->last_sa(); return CAPS_SA_OK; });
}
int CAPS_API(shard_fix_first_lcp)(caps_sa_shard* s, uint64_t prev_sa, void* dLCP)
{
    if (!s) return caps::fail(CAPS_SA_EINVAL, "null shard");
    return caps::guarded([&]() -> int { s->impl->fix_first_lcp(prev_sa, dLCP); return CAPS_SA_OK; });
}

}  // extern "C"

#if defined(CAPS_PHASE_CLOCK) && !defined(CAPS_EMUL)
// measurement builds only (kernels.h PHASE_MARK): copies the 32 phase counters out and clears them
extern "C" __attribute__((visibility("default"))) int caps_sa_hip_phase_clock(uint64_t* out32)
{
    unsigned long long h[32];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(caps::caps_phase_clock), sizeof(h)) != hipSuccess) return -1;
    for (int i = 0; i < 32; ++i) out32[i] = h[i];
    for (int i = 0; i < 32; ++i) h[i] = 0;
    return hipMemcpyToSymbol(HIP_SYMBOL(caps::caps_phase_clock), h, sizeof(h)) == hipSuccess ? 0 : -1;
}
#endif

#if defined(CAPS_EQ_CHECK) && !defined(CAPS_EMUL)
// debugging builds only (kernels.h EQ_OK): copies the 64 check counters out and clears them
extern "C" __attribute__((visibility("default"))) int caps_sa_hip_eq_check(uint32_t* out64)
{
    unsigned int h[64];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(caps::caps_eq_check), sizeof(h)) != hipSuccess) return -1;
    for (int i = 0; i < 64; ++i) out64[i] = h[i];
    for (int i = 0; i < 64; ++i) h[i] = 0;
    return hipMemcpyToSymbol(HIP_SYMBOL(caps::caps_eq_check), h, sizeof(h)) == hipSuccess ? 0 : -1;
}
#endif
