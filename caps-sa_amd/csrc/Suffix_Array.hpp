// caps-sa_amd/csrc/Suffix_Array.hpp
//
// Host-side C++ mirror of the reference's class surface CaPS_SA::Suffix_Array<T_idx_>
// (reference include/Suffix_Array.hpp:148-181): same constructor arguments, same
// accessors, same dump format -- but construct() hands the whole samplesort to the
// MI355X through the C ABI of include/caps_sa_hip.h (libcaps_sa_hip.so).  A program
// written against the reference header (e.g. its CLI, src/main.cpp:78-80) compiles
// against this one unchanged.
//
// Differences, all deliberate:
//  * errors: the reference calls std::exit (src/Suffix_Array.cpp:33-37); construct()
//    here throws std::runtime_error carrying caps_sa_hip_last_error();
//  * valid for every n >= 0 (the reference divides by zero for n < 32 / p_eff < 2);
//  * bounded max_context (0 < max_context < n) runs the reference's own merge sequence on ONE device (csrc/bounded.h);
//  * SA_ / LCP_ are page-locked (caps_sa_hip_host_alloc) when the driver grants it, plain malloc otherwise: the
//    results then leave the GPU at the PCIe link rate (C2: 38 ms instead of 88 ms for the two arrays) -- like the
//    reference's mallocs (src/Suffix_Array.cpp:20-21) the allocation belongs to the constructor, not to construct();
//  * an optional list of devices: construct() then shards the build over them (caps_sa_hip_build_multi_*);
//  * construct_bwt() (not in the reference): construct() plus the Burrows-Wheeler transform (include/caps_sa_hip.h), one device;
//    its n-byte buffer is allocated by the first construct_bwt(), so construct() callers pay nothing for it.
//  * kmers() / kmer_spectrum() / kmer_census() (not in the reference): the k-mer table, spectrum and census of the text from SA() and LCP()
//    after a full-context construct() (include/caps_sa_hip.h "k-mers from SA and LCP").
//  * lpf() / lz77() (not in the reference): the longest-previous-factor array with a previous occurrence for every position, and the LZ77
//    factorization, from SA() and LCP() after a full-context construct() (include/caps_sa_hip.h "LPF and LZ77 from SA and LCP").
//  * ISA() (not in the reference): the inverse suffix array, after a full-context construct() (include/caps_sa_hip.h "ISA and longest
//    common extensions"); and the class LCE_Index: batched longest common extensions and range minima over LCP from one blob.
//  * cross_mums() / cross_mems() / longest_common_substring() (not in the reference): the maximal unique matches, the rare maximal exact
//    matches and the longest common substring between T()[0 .. split) and T()[split .. n), from SA(), LCP() and the BWT after a
//    full-context construct() / construct_bwt() (include/caps_sa_hip.h "MUMs and MEMs between two texts").
//  * collection_kmers() / kmer_sharing() (not in the reference): the k-mers of up to 64 documents inside T() with the set of documents
//    that hold each, and how many every pair of documents shares (include/caps_sa_hip.h "k-mers across a collection").
//  * the free function inverse_bwt() (not in the reference): the text back from (BWT, primary).
//  * the class FM_Index (not in the reference either): count, locate, matching statistics, MEMs and extract over (BWT, primary) and a sample of the SA.
#ifndef CAPS_SA_AMD_SUFFIX_ARRAY_HPP
#define CAPS_SA_AMD_SUFFIX_ARRAY_HPP

#include <algorithm>
#include <cstdint>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <new>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/caps_sa_hip.h"

namespace CaPS_SA
{

template <typename T_idx_>
class Suffix_Array
{
    static_assert(std::is_same<T_idx_, uint32_t>::value || std::is_same<T_idx_, uint64_t>::value,
                  "instantiated for uint32_t and uint64_t like the reference (src/Suffix_Array.cpp:543-544)");

public:
    typedef T_idx_ idx_t;

    // Reference: include/Suffix_Array.hpp:155, src/Suffix_Array.cpp:16-38.  T is borrowed
    // and must outlive the object; SA/LCP are allocated here and freed by the destructor.
    Suffix_Array(const char* T, idx_t n, idx_t subproblem_count = 0, idx_t max_context = 0, int device = 0)
        : Suffix_Array(T, n, subproblem_count, max_context, std::vector<int>(1, device)) {}

    // devices: HIP device ordinals the build is sharded over (one: the single-GPU build)
    Suffix_Array(const char* T, idx_t n, idx_t subproblem_count, idx_t max_context, const std::vector<int>& devices)
        : T_(T), n_(n), SA_(nullptr), LCP_(nullptr), pinned_(false), BWT_(nullptr), bwt_pinned_(false), primary_(UINT64_MAX),
          subproblem_count_(subproblem_count), max_context_(max_context), devices_(devices), stats_()
    {
        if (devices_.empty()) throw std::invalid_argument("Suffix_Array: no devices");
        const std::size_t bytes = (n ? static_cast<std::size_t>(n) : 1) * sizeof(idx_t);
        SA_ = static_cast<idx_t*>(caps_sa_hip_host_alloc(bytes));
        LCP_ = SA_ ? static_cast<idx_t*>(caps_sa_hip_host_alloc(bytes)) : nullptr;
        pinned_ = SA_ && LCP_;
        if (!pinned_) {                                       // no GPU / no page-locked memory to be had: pageable
            if (SA_) caps_sa_hip_host_free(SA_);
            SA_ = static_cast<idx_t*>(std::malloc(bytes));
            LCP_ = static_cast<idx_t*>(std::malloc(bytes));
            if (!SA_ || !LCP_) { std::free(SA_); std::free(LCP_); throw std::bad_alloc(); }
        }
    }

    Suffix_Array(const Suffix_Array&) = delete;                 // hpp:157-160
    Suffix_Array& operator=(const Suffix_Array&) = delete;
    Suffix_Array(Suffix_Array&&) = delete;
    Suffix_Array& operator=(Suffix_Array&&) = delete;

    ~Suffix_Array()                                             // cpp:41-45
    {
        if (pinned_) { caps_sa_hip_host_free(SA_); caps_sa_hip_host_free(LCP_); }
        else { std::free(SA_); std::free(LCP_); }
        if (bwt_pinned_) caps_sa_hip_host_free(BWT_);
        else std::free(BWT_);
    }

    const char* T() const { return T_; }                        // hpp:165
    idx_t n() const { return n_; }                              // hpp:168
    const idx_t* SA() const { return SA_; }                     // hpp:171
    const idx_t* LCP() const { return LCP_; }                   // hpp:174

    // Reference: src/Suffix_Array.cpp:466-494.  May be called more than once.
    void construct()
    {
        int rc;
        const int nd = static_cast<int>(devices_.size());
        if (std::is_same<idx_t, uint32_t>::value)
            rc = caps_sa_hip_build_multi_u32(T_, n_, subproblem_count_, max_context_, reinterpret_cast<uint32_t*>(SA_),
                                             reinterpret_cast<uint32_t*>(LCP_), devices_.data(), nd, &stats_);
        else
            rc = caps_sa_hip_build_multi_u64(T_, n_, subproblem_count_, max_context_, reinterpret_cast<uint64_t*>(SA_),
                                             reinterpret_cast<uint64_t*>(LCP_), devices_.data(), nd, &stats_);
        if (rc != CAPS_SA_OK)
            throw std::runtime_error(std::string("caps_sa_hip_build: ") + caps_sa_hip_last_error());
    }

    // construct() plus the BWT: BWT()[k] = T[(SA[k] + n - 1) mod n], primary() = the k with SA[k] == 0 (UINT64_MAX for n = 0).
    // One device only (the sharded build has no BWT output): throws std::invalid_argument with more.
    void construct_bwt()
    {
        if (devices_.size() != 1) throw std::invalid_argument("Suffix_Array::construct_bwt: one device only (the sharded build has no BWT)");
        if (!BWT_) {                                          // on first use, page-locked when the driver grants it (like SA_ / LCP_)
            const std::size_t bytes = n_ ? static_cast<std::size_t>(n_) : 1;
            BWT_ = static_cast<uint8_t*>(caps_sa_hip_host_alloc(bytes));
            bwt_pinned_ = BWT_ != nullptr;
            if (!BWT_) BWT_ = static_cast<uint8_t*>(std::malloc(bytes));
            if (!BWT_) throw std::bad_alloc();
        }
        int rc;
        if (std::is_same<idx_t, uint32_t>::value)
            rc = caps_sa_hip_build_bwt_u32(T_, n_, subproblem_count_, max_context_, reinterpret_cast<uint32_t*>(SA_),
                                           reinterpret_cast<uint32_t*>(LCP_), BWT_, &primary_, devices_[0], &stats_);
        else
            rc = caps_sa_hip_build_bwt_u64(T_, n_, subproblem_count_, max_context_, reinterpret_cast<uint64_t*>(SA_),
                                           reinterpret_cast<uint64_t*>(LCP_), BWT_, &primary_, devices_[0], &stats_);
        if (rc != CAPS_SA_OK)
            throw std::runtime_error(std::string("caps_sa_hip_build_bwt: ") + caps_sa_hip_last_error());
    }
    const uint8_t* BWT() const { return BWT_; }                 // null before the first construct_bwt()
    uint64_t primary() const { return primary_; }

    // ---- k-mers from SA and LCP (include/caps_sa_hip.h; not in the reference).  After a full-context construct() / construct_bwt():
    // with max_context set the arrays are no suffix array and these throw std::invalid_argument.  On devices()[0].
    struct Kmer { uint64_t first, count, pos; };               // the ABI's 24-byte record: the k-mer is T()[pos .. pos + k), at SA()[first .. first + count)
    // the distinct k-mers with min_count <= count (<= max_count unless that is 0), in the library's byte order
    std::vector<Kmer> kmers(uint64_t k, uint64_t min_count = 1, uint64_t max_count = 0) const
    {
        kmer_arrays_ok("kmers");
        static_assert(sizeof(Kmer) == 24, "the ABI's record");
        uint64_t found = 0;
        kmers_call(k, min_count, max_count, nullptr, 0, &found);                 // the counting call
        std::vector<Kmer> out(static_cast<std::size_t>(found));
        if (found) kmers_call(k, min_count, max_count, out.data(), found, &found);
        return out;
    }
    // hist[c] = the distinct k-mers that occur c times (1 <= c < bins), hist[bins] = bins times or more, hist[0] = 0
    std::vector<uint64_t> kmer_spectrum(uint64_t k, uint32_t bins = 1024) const
    {
        kmer_arrays_ok("kmer_spectrum");
        std::vector<uint64_t> hist(static_cast<std::size_t>(bins) + 1, 0);
        const int rc = std::is_same<idx_t, uint32_t>::value
            ? caps_sa_hip_kmer_spectrum_u32(reinterpret_cast<const uint32_t*>(SA_), reinterpret_cast<const uint32_t*>(LCP_), n_, k, bins, hist.data(), devices_[0])
            : caps_sa_hip_kmer_spectrum_u64(reinterpret_cast<const uint64_t*>(SA_), reinterpret_cast<const uint64_t*>(LCP_), n_, k, bins, hist.data(), devices_[0]);
        if (rc != CAPS_SA_OK) throw std::runtime_error(std::string("caps_sa_hip_kmer_spectrum: ") + caps_sa_hip_last_error());
        return hist;
    }
    // distinct[k] / unique[k], k = 1 .. max_k: the number of distinct k-mers and of those that occur once (index 0 is 0)
    void kmer_census(uint32_t max_k, std::vector<uint64_t>& distinct, std::vector<uint64_t>& unique) const
    {
        kmer_arrays_ok("kmer_census");
        distinct.assign(static_cast<std::size_t>(max_k) + 1, 0);
        unique.assign(static_cast<std::size_t>(max_k) + 1, 0);
        const int rc = std::is_same<idx_t, uint32_t>::value
            ? caps_sa_hip_kmer_census_u32(reinterpret_cast<const uint32_t*>(SA_), reinterpret_cast<const uint32_t*>(LCP_), n_, max_k, distinct.data(), unique.data(), devices_[0])
            : caps_sa_hip_kmer_census_u64(reinterpret_cast<const uint64_t*>(SA_), reinterpret_cast<const uint64_t*>(LCP_), n_, max_k, distinct.data(), unique.data(), devices_[0]);
        if (rc != CAPS_SA_OK) throw std::runtime_error(std::string("caps_sa_hip_kmer_census: ") + caps_sa_hip_last_error());
    }

    // ---- k-mers across a collection (include/caps_sa_hip.h; not in the reference).  docs: up to 64 ascending, disjoint (start, length)
    // in T().  After a full-context construct() / construct_bwt(); with max_context set these throw std::invalid_argument.  On devices()[0].
    struct Coll_Kmer { uint64_t first, count, occ, docs; };    // the ABI's 32-byte record: T()[SA()[first] .. + k), in the documents of the mask `docs`
    typedef std::vector<std::pair<uint64_t, uint64_t>> Documents;
    // the k-mers inside a document whose set of documents has min_docs .. max_docs members (0: no upper bound), all of all_of, none of none_of
    std::vector<Coll_Kmer> collection_kmers(uint64_t k, const Documents& docs, uint64_t min_docs = 1, uint64_t max_docs = 0, uint64_t all_of = 0,
                                            uint64_t none_of = 0) const
    {
        kmer_arrays_ok("collection_kmers");
        static_assert(sizeof(Coll_Kmer) == 32, "the ABI's record");
        std::vector<uint64_t> st, ln;
        for (const auto& d : docs) { st.push_back(d.first); ln.push_back(d.second); }
        const uint32_t m = static_cast<uint32_t>(docs.size());
        auto call = [&](void* records, uint64_t capacity, uint64_t* found) {
            const int rc = std::is_same<idx_t, uint32_t>::value
                ? caps_sa_hip_coll_kmers_u32(reinterpret_cast<const uint32_t*>(SA_), reinterpret_cast<const uint32_t*>(LCP_), n_, k, st.data(), ln.data(), m, min_docs, max_docs, all_of, none_of, records, capacity, found, devices_[0])
                : caps_sa_hip_coll_kmers_u64(reinterpret_cast<const uint64_t*>(SA_), reinterpret_cast<const uint64_t*>(LCP_), n_, k, st.data(), ln.data(), m, min_docs, max_docs, all_of, none_of, records, capacity, found, devices_[0]);
            if (rc != CAPS_SA_OK) throw std::runtime_error(std::string("caps_sa_hip_coll_kmers: ") + caps_sa_hip_last_error());
        };
        uint64_t found = 0;
        call(nullptr, 0, &found);                                                // the counting call
        std::vector<Coll_Kmer> out(static_cast<std::size_t>(found));
        if (found) call(out.data(), found, &found);
        return out;
    }
    // freq[c], c = 0 .. 64: the k-mers of the collection in exactly c documents; shared[a * m + b]: those in both a and b
    void kmer_sharing(uint64_t k, const Documents& docs, std::vector<uint64_t>& freq, std::vector<uint64_t>& shared) const
    {
        kmer_arrays_ok("kmer_sharing");
        std::vector<uint64_t> st, ln;
        for (const auto& d : docs) { st.push_back(d.first); ln.push_back(d.second); }
        const uint32_t m = static_cast<uint32_t>(docs.size());
        freq.assign(65, 0);
        shared.assign(static_cast<std::size_t>(m) * m, 0);
        const int rc = std::is_same<idx_t, uint32_t>::value
            ? caps_sa_hip_coll_sharing_u32(reinterpret_cast<const uint32_t*>(SA_), reinterpret_cast<const uint32_t*>(LCP_), n_, k, st.data(), ln.data(), m, freq.data(), shared.data(), devices_[0])
            : caps_sa_hip_coll_sharing_u64(reinterpret_cast<const uint64_t*>(SA_), reinterpret_cast<const uint64_t*>(LCP_), n_, k, st.data(), ln.data(), m, freq.data(), shared.data(), devices_[0]);
        if (rc != CAPS_SA_OK) throw std::runtime_error(std::string("caps_sa_hip_coll_sharing: ") + caps_sa_hip_last_error());
    }

    // ---- LPF and LZ77 from SA and LCP (include/caps_sa_hip.h; not in the reference).  After a full-context construct() / construct_bwt():
    // with max_context set these throw std::invalid_argument.  On devices()[0].
    struct Phrase { uint64_t pos, len, src; };                 // the ABI's 24-byte record: T()[src .. src + len), or the byte T()[pos] where src == literal
    static constexpr uint64_t literal = ~static_cast<uint64_t>(0);
    // LPF[i] = the longest prefix of T()[i ..) that also starts at some j < i, Prev[i] = such a j (all ones where LPF[i] = 0), text order
    void lpf(std::vector<idx_t>& LPF, std::vector<idx_t>& Prev) const
    {
        lz_arrays_ok("lpf");
        LPF.assign(static_cast<std::size_t>(n_), 0);
        Prev.assign(static_cast<std::size_t>(n_), static_cast<idx_t>(~static_cast<idx_t>(0)));
        const int rc = std::is_same<idx_t, uint32_t>::value
            ? caps_sa_hip_lpf_u32(reinterpret_cast<const uint32_t*>(SA_), reinterpret_cast<const uint32_t*>(LCP_), n_, reinterpret_cast<uint32_t*>(LPF.data()), reinterpret_cast<uint32_t*>(Prev.data()), devices_[0])
            : caps_sa_hip_lpf_u64(reinterpret_cast<const uint64_t*>(SA_), reinterpret_cast<const uint64_t*>(LCP_), n_, reinterpret_cast<uint64_t*>(LPF.data()), reinterpret_cast<uint64_t*>(Prev.data()), devices_[0]);
        if (rc != CAPS_SA_OK) throw std::runtime_error(std::string("caps_sa_hip_lpf: ") + caps_sa_hip_last_error());
    }
    // the phrases in text order.  One call (arrays up, lpf, count, write) into room for min(n, n / 8 + 1024) records, enough wherever the
    // phrases average 8 bytes or more; only where it is not, a second call with the exact number (which runs lpf again)
    std::vector<Phrase> lz77() const
    {
        lz_arrays_ok("lz77");
        static_assert(sizeof(Phrase) == 24, "the ABI's record");
        const uint64_t n = static_cast<uint64_t>(n_);
        uint64_t z = 0;
        std::vector<Phrase> out(static_cast<std::size_t>(std::min<uint64_t>(n, n / 8 + 1024)));
        if (!lz77_call(out.empty() ? nullptr : out.data(), out.size(), &z)) {
            out.assign(static_cast<std::size_t>(z), Phrase{});
            if (!lz77_call(out.data(), z, &z)) throw std::runtime_error(std::string("caps_sa_hip_lz77: ") + caps_sa_hip_last_error());
        }
        out.resize(static_cast<std::size_t>(z));
        return out;
    }

    // ---- MUMs and MEMs between two texts (include/caps_sa_hip.h "MUMs and MEMs between two texts"; not in the reference).  T() = A . sep . B
    // with the separator -- a byte that occurs nowhere else -- at split - 1.  After a full-context construct() / construct_bwt(): with
    // max_context set these throw std::invalid_argument.  The BWT is construct_bwt()'s; after a plain construct() it is gathered from T()
    // and SA() on the host at the first call.  On devices()[0].
    struct Match { uint64_t a, b, len; };                      // the ABI's 24-byte record: T()[a .. a + len) == T()[b .. b + len), a < split <= b
    struct Cross_Summary { uint64_t records, skipped_runs, lcs_len, lcs_a, lcs_b; };
    static constexpr uint32_t cross_max_occ = CAPS_SA_CROSS_MAX_OCC;
    // the maximal unique matches of at least min_len bytes, in rank order
    std::vector<Match> cross_mums(uint64_t split, uint64_t min_len = 1, Cross_Summary* summary = nullptr) const
    {
        return cross(false, split, min_len, 0, summary);
    }
    // every maximal exact match of at least min_len bytes whose first min_len bytes occur at most max_occ (2 .. 64) times in T(); the
    // summary's skipped_runs counts the more frequent seeds that were left out
    std::vector<Match> cross_mems(uint64_t split, uint64_t min_len = 1, uint32_t max_occ = CAPS_SA_CROSS_MAX_OCC, Cross_Summary* summary = nullptr) const
    {
        return cross(true, split, min_len, max_occ, summary);
    }
    // the longest common substring of T()[0 .. split) and T()[split .. n): a = the position in the first side; len 0: none
    Match longest_common_substring(uint64_t split) const
    {
        Cross_Summary s{};
        cross(false, split, std::max<uint64_t>(static_cast<uint64_t>(n_), 1), 0, &s);
        return Match{s.lcs_a, s.lcs_b, s.lcs_len};
    }

    // ---- the inverse suffix array (include/caps_sa_hip.h "ISA and longest common extensions"; not in the reference): ISA()[SA()[r]] = r.
    // After a full-context construct(); with max_context set it throws std::invalid_argument.  On devices()[0].
    std::vector<idx_t> ISA() const
    {
        if (max_context_ != 0 && max_context_ < n_)
            throw std::invalid_argument("Suffix_Array::ISA: the inverse needs a full-context suffix array (max_context is set)");
        std::vector<idx_t> out(static_cast<std::size_t>(n_));
        const int rc = std::is_same<idx_t, uint32_t>::value
            ? caps_sa_hip_isa_u32(reinterpret_cast<const uint32_t*>(SA_), n_, reinterpret_cast<uint32_t*>(out.data()), devices_[0])
            : caps_sa_hip_isa_u64(reinterpret_cast<const uint64_t*>(SA_), n_, reinterpret_cast<uint64_t*>(out.data()), devices_[0]);
        if (rc != CAPS_SA_OK) throw std::runtime_error(std::string("caps_sa_hip_isa: ") + caps_sa_hip_last_error());
        return out;
    }
    bool full_context() const { return max_context_ == 0 || max_context_ >= n_; }
    int device() const { return devices_[0]; }

    // Reference: src/Suffix_Array.cpp:497-509 -- u64 n, then SA, then LCP, native endianness.
    void dump(std::ofstream& output)
    {
        const std::size_t n = n_;
        output.write(reinterpret_cast<const char*>(&n), sizeof(std::size_t));
        output.write(reinterpret_cast<const char*>(SA_), n * sizeof(idx_t));
        output.write(reinterpret_cast<const char*>(LCP_), n * sizeof(idx_t));
    }

    // Per-phase record of the last construct() (replaces the reference's stderr timing lines).
    const caps_sa_stats& stats() const { return stats_; }

private:
    void kmer_arrays_ok(const char* what) const
    {
        if (max_context_ != 0 && max_context_ < n_)
            throw std::invalid_argument(std::string("Suffix_Array::") + what + ": k-mers need a full-context suffix array (max_context is set)");
    }
    void kmers_call(uint64_t k, uint64_t min_count, uint64_t max_count, void* records, uint64_t capacity, uint64_t* found) const
    {
        const int rc = std::is_same<idx_t, uint32_t>::value
            ? caps_sa_hip_kmers_u32(reinterpret_cast<const uint32_t*>(SA_), reinterpret_cast<const uint32_t*>(LCP_), n_, k, min_count, max_count, records, capacity, found, devices_[0])
            : caps_sa_hip_kmers_u64(reinterpret_cast<const uint64_t*>(SA_), reinterpret_cast<const uint64_t*>(LCP_), n_, k, min_count, max_count, records, capacity, found, devices_[0]);
        if (rc != CAPS_SA_OK) throw std::runtime_error(std::string("caps_sa_hip_kmers: ") + caps_sa_hip_last_error());
    }

    void lz_arrays_ok(const char* what) const
    {
        if (max_context_ != 0 && max_context_ < n_)
            throw std::invalid_argument(std::string("Suffix_Array::") + what + ": LPF and LZ77 need a full-context suffix array (max_context is set)");
    }
    // false: the buffer was too small and *z says how many records there are; any other failure throws
    bool lz77_call(void* records, uint64_t capacity, uint64_t* z) const
    {
        const int rc = std::is_same<idx_t, uint32_t>::value
            ? caps_sa_hip_lz77_u32(reinterpret_cast<const uint32_t*>(SA_), reinterpret_cast<const uint32_t*>(LCP_), n_, records, capacity, z, devices_[0])
            : caps_sa_hip_lz77_u64(reinterpret_cast<const uint64_t*>(SA_), reinterpret_cast<const uint64_t*>(LCP_), n_, records, capacity, z, devices_[0]);
        if (rc != CAPS_SA_OK && records && *z > capacity) return false;
        if (rc != CAPS_SA_OK) throw std::runtime_error(std::string("caps_sa_hip_lz77: ") + caps_sa_hip_last_error());
        return true;
    }

    // false: the buffer was too small and the summary says how many records there are; any other failure throws
    bool cross_call(bool mems, const uint8_t* bwt, uint64_t split, uint64_t min_len, uint32_t max_occ, void* records, uint64_t capacity, uint64_t* summary) const
    {
        const uint32_t* s32 = reinterpret_cast<const uint32_t*>(SA_);
        const uint32_t* l32 = reinterpret_cast<const uint32_t*>(LCP_);
        const uint64_t* s64 = reinterpret_cast<const uint64_t*>(SA_);
        const uint64_t* l64 = reinterpret_cast<const uint64_t*>(LCP_);
        const bool narrow = std::is_same<idx_t, uint32_t>::value;
        const int rc = mems
            ? (narrow ? caps_sa_hip_cross_mems_u32(s32, l32, bwt, n_, split, min_len, max_occ, records, capacity, summary, devices_[0])
                      : caps_sa_hip_cross_mems_u64(s64, l64, bwt, n_, split, min_len, max_occ, records, capacity, summary, devices_[0]))
            : (narrow ? caps_sa_hip_cross_mums_u32(s32, l32, bwt, n_, split, min_len, records, capacity, summary, devices_[0])
                      : caps_sa_hip_cross_mums_u64(s64, l64, bwt, n_, split, min_len, records, capacity, summary, devices_[0]));
        if (rc != CAPS_SA_OK && records && summary[0] > capacity) return false;
        if (rc != CAPS_SA_OK) throw std::runtime_error(std::string(mems ? "caps_sa_hip_cross_mems: " : "caps_sa_hip_cross_mums: ") + caps_sa_hip_last_error());
        return true;
    }
    std::vector<Match> cross(bool mems, uint64_t split, uint64_t min_len, uint32_t max_occ, Cross_Summary* out) const
    {
        static_assert(sizeof(Match) == 24, "the ABI's record");
        if (max_context_ != 0 && max_context_ < n_)
            throw std::invalid_argument(std::string("Suffix_Array::") + (mems ? "cross_mems" : "cross_mums") + ": MUMs and MEMs need a full-context suffix array (max_context is set)");
        if (!SA_ || !LCP_) throw std::logic_error("Suffix_Array: construct() has not been called");
        const uint8_t* bwt = BWT_;
        if (!bwt) {
            const std::size_t n = static_cast<std::size_t>(n_);
            if (cross_bwt_.size() != n) {
                cross_bwt_.resize(n);
                for (std::size_t r = 0; r < n; ++r) cross_bwt_[r] = static_cast<uint8_t>(T_[SA_[r] ? static_cast<std::size_t>(SA_[r]) - 1 : n - 1]);
            }
            bwt = cross_bwt_.data();
        }
        uint64_t summary[8] = {0};
        cross_call(mems, bwt, split, min_len, max_occ, nullptr, 0, summary);      // the counting call
        std::vector<Match> rec(static_cast<std::size_t>(summary[0]));
        if (!rec.empty() && !cross_call(mems, bwt, split, min_len, max_occ, rec.data(), rec.size(), summary))
            throw std::runtime_error("caps_sa_hip_cross: the counting call and the writing call disagree");
        if (out) *out = Cross_Summary{summary[0], summary[1], summary[2], summary[3], summary[4]};
        return rec;
    }
    mutable std::vector<uint8_t> cross_bwt_;                    // the BWT gathered for cross_* after a plain construct()

    const char* const T_;
    const idx_t n_;
    idx_t* SA_;
    idx_t* LCP_;
    bool pinned_;
    uint8_t* BWT_;
    bool bwt_pinned_;
    uint64_t primary_;
    const idx_t subproblem_count_;
    const idx_t max_context_;
    const std::vector<int> devices_;
    caps_sa_stats stats_;
};

// The text back from its BWT (include/caps_sa_hip.h caps_sa_hip_inverse_bwt_*; not in the reference): BWT and primary as
// construct_bwt() returns them, T receives n bytes.  32-bit indices for n <= UINT32_MAX, else 64-bit; throws std::runtime_error
// on any error, an input that is not the BWT of a text included.
inline void inverse_bwt(const uint8_t* BWT, uint64_t n, uint64_t primary, char* T, int device = 0)
{
    const int rc = n <= UINT32_MAX ? caps_sa_hip_inverse_bwt_u32(BWT, n, primary, T, device)
                                   : caps_sa_hip_inverse_bwt_u64(BWT, n, primary, T, device);
    if (rc != CAPS_SA_OK)
        throw std::runtime_error(std::string(n <= UINT32_MAX ? "caps_sa_hip_inverse_bwt_u32: " : "caps_sa_hip_inverse_bwt_u64: ") +
                                 caps_sa_hip_last_error());
}

// FM-index over (BWT, primary) (include/caps_sa_hip.h "FM-index"; not in the reference): count and locate for batches of patterns,
// extract for batches of text ranges (after add_text_samples), over texts of at most 4 distinct bytes.  The index is one blob (data(), size()); save / load write and read exactly it.  Every
// error of the C ABI is thrown as std::runtime_error with its message.  build_wide makes the wide format (include/caps_sa_hip.h
// "FM-index: the wide format") for 1 .. 256 distinct bytes: count, locate, matching_statistics and mems work on either blob,
// add_text_samples and extract throw the ABI's error on a wide one.
class FM_Index
{
public:
    FM_Index() : device_(0) {}

    // SA: null (an index that counts), or the whole suffix array, idx_t = uint32_t / uint64_t (it also locates)
    template <typename idx_t>
    static FM_Index build(const uint8_t* BWT, uint64_t n, uint64_t primary, const idx_t* SA, uint32_t sa_sample = 32, int device = 0)
    {
        static_assert(std::is_same<idx_t, uint32_t>::value || std::is_same<idx_t, uint64_t>::value, "uint32_t or uint64_t");
        FM_Index fm;
        fm.device_ = device;
        uint64_t bytes = 0;
        check(caps_sa_hip_fm_index_bytes(n, SA ? sa_sample : 0, (int)sizeof(idx_t), &bytes), "caps_sa_hip_fm_index_bytes");
        fm.blob_.resize(static_cast<std::size_t>(bytes));
        if (sizeof(idx_t) == 4)
            check(caps_sa_hip_fm_build_u32(BWT, n, primary, reinterpret_cast<const uint32_t*>(SA), sa_sample, fm.blob_.data(), bytes, device),
                  "caps_sa_hip_fm_build_u32");
        else
            check(caps_sa_hip_fm_build_u64(BWT, n, primary, reinterpret_cast<const uint64_t*>(SA), sa_sample, fm.blob_.data(), bytes, device),
                  "caps_sa_hip_fm_build_u64");
        return fm;
    }

    // The index WITH samples from (BWT, primary) alone (include/caps_sa_hip.h "FM-index from the BWT alone"): the same blob as
    // build() with the suffix array of the text the BWT inverts to.  32-bit indices for n <= UINT32_MAX, else 64-bit.
    static FM_Index build_from_bwt(const uint8_t* BWT, uint64_t n, uint64_t primary, uint32_t sa_sample = 32, int device = 0)
    {
        FM_Index fm;
        fm.device_ = device;
        const bool narrow = n <= UINT32_MAX;
        uint64_t bytes = 0;
        check(caps_sa_hip_fm_index_bytes(n, sa_sample, narrow ? 4 : 8, &bytes), "caps_sa_hip_fm_index_bytes");
        fm.blob_.resize(static_cast<std::size_t>(bytes));
        if (narrow)
            check(caps_sa_hip_fm_build_from_bwt_u32(BWT, n, primary, sa_sample, fm.blob_.data(), bytes, device), "caps_sa_hip_fm_build_from_bwt_u32");
        else
            check(caps_sa_hip_fm_build_from_bwt_u64(BWT, n, primary, sa_sample, fm.blob_.data(), bytes, device), "caps_sa_hip_fm_build_from_bwt_u64");
        return fm;
    }

    // The wide format, for a BWT of 1 .. 256 distinct bytes; SA as in build().  The blob is sized for the bytes that occur (counted
    // here, one pass over the BWT) and cut to the size the library reports in its header.
    template <typename idx_t>
    static FM_Index build_wide(const uint8_t* BWT, uint64_t n, uint64_t primary, const idx_t* SA, uint32_t sa_sample = 32, int device = 0)
    {
        static_assert(std::is_same<idx_t, uint32_t>::value || std::is_same<idx_t, uint64_t>::value, "uint32_t or uint64_t");
        FM_Index fm;
        fm.device_ = device;
        bool seen[256] = {};
        uint32_t sigma = 0;
        if (BWT)
            for (uint64_t i = 0; i < n; ++i)
                if (!seen[BWT[i]]) { seen[BWT[i]] = true; ++sigma; }
        uint64_t bytes = 0;
        check(caps_sa_hip_fm_wide_index_bytes(n, sigma, SA ? sa_sample : 0, (int)sizeof(idx_t), &bytes), "caps_sa_hip_fm_wide_index_bytes");
        fm.blob_.resize(static_cast<std::size_t>(bytes));
        if (sizeof(idx_t) == 4)
            check(caps_sa_hip_fm_build_wide_u32(BWT, n, primary, reinterpret_cast<const uint32_t*>(SA), sa_sample, fm.blob_.data(), bytes, device),
                  "caps_sa_hip_fm_build_wide_u32");
        else
            check(caps_sa_hip_fm_build_wide_u64(BWT, n, primary, reinterpret_cast<const uint64_t*>(SA), sa_sample, fm.blob_.data(), bytes, device),
                  "caps_sa_hip_fm_build_wide_u64");
        uint64_t total = 0;
        std::memcpy(&total, fm.blob_.data() + 18 * 8, 8);      // header word 18: the blob's size
        if (total <= bytes) fm.blob_.resize(static_cast<std::size_t>(total));
        return fm;
    }

    const uint8_t* data() const { return blob_.data(); }
    std::size_t size() const { return blob_.size(); }
    bool wide() const { return blob_.size() >= 256 && std::memcmp(blob_.data(), "CAPSFMW1", 8) == 0; }
    // the number of distinct bytes of the text (header word 5 of both formats)
    uint32_t sigma() const
    {
        uint64_t v = 0;
        if (blob_.size() >= 256) std::memcpy(&v, blob_.data() + 40, 8);
        return static_cast<uint32_t>(v);
    }

    // patterns: the concatenated bytes, off[j] .. off[j + 1] the j-th of them (off.size() = q + 1) -> first / count, q entries each
    void count(const std::string& patterns, const std::vector<uint64_t>& off, std::vector<uint64_t>& first, std::vector<uint64_t>& cnt) const
    {
        const uint64_t q = off.empty() ? 0 : off.size() - 1;
        first.assign(q, 0);
        cnt.assign(q, 0);
        check(caps_sa_hip_fm_count(blob_.data(), blob_.size(), reinterpret_cast<const uint8_t*>(patterns.data()), off.data(), q,
                                   first.data(), cnt.data(), device_), "caps_sa_hip_fm_count");
    }

    // at most max_hits positions per query, in SA order: pos[out_off[j] .. out_off[j + 1])
    void locate(const std::vector<uint64_t>& first, const std::vector<uint64_t>& cnt, uint64_t max_hits, std::vector<uint64_t>& out_off,
                std::vector<uint64_t>& pos) const
    {
        const uint64_t q = first.size();
        out_off.assign(q + 1, 0);
        for (uint64_t j = 0; j < q; ++j) out_off[j + 1] = out_off[j] + (cnt[j] < max_hits ? cnt[j] : max_hits);
        pos.assign(static_cast<std::size_t>(out_off[q]), 0);
        check(caps_sa_hip_fm_locate(blob_.data(), blob_.size(), first.data(), cnt.data(), out_off.data(), q, pos.data(), device_),
              "caps_sa_hip_fm_locate");
    }

    // Matching statistics (include/caps_sa_hip.h "FM-index: matching statistics"): slot off[j] - off[0] + e - 1 of len = L[e] of
    // pattern j, the longest piece ending at e that occurs in the text (at most max_len when max_len > 0); first / cnt: its SA
    // interval, or null: not computed.  Needs no SA samples.
    void matching_statistics(const std::string& patterns, const std::vector<uint64_t>& off, std::vector<uint32_t>& len,
                             std::vector<uint64_t>* first = nullptr, std::vector<uint64_t>* cnt = nullptr, uint32_t max_len = 0) const
    {
        const uint64_t q = off.empty() ? 0 : off.size() - 1, total = q ? off[q] - off[0] : 0;
        len.assign(static_cast<std::size_t>(total), 0);
        if (first) first->assign(static_cast<std::size_t>(total), 0);
        if (cnt) cnt->assign(static_cast<std::size_t>(total), 0);
        check(caps_sa_hip_fm_match(blob_.data(), blob_.size(), reinterpret_cast<const uint8_t*>(patterns.data()), off.data(), q, max_len,
                                   len.data(), first ? first->data() : nullptr, cnt ? cnt->data() : nullptr, device_), "caps_sa_hip_fm_match");
    }

    // A maximal exact match: P[start .. start + length) of pattern `pattern` occurs at SA[first .. first + count) and can be
    // extended neither to the left nor to the right.  The 32-byte record of the C ABI.
    struct Mem {
        uint64_t pattern;
        uint32_t start, length;
        uint64_t first, count;
    };

    // The MEMs of at least min_len bytes in (pattern, increasing end) order; mems[mem_off[j] .. mem_off[j + 1]) are pattern j's.
    // The counting call, then the writing call.
    void mems(const std::string& patterns, const std::vector<uint64_t>& off, uint32_t min_len, std::vector<uint64_t>& mem_off,
              std::vector<Mem>& mems) const
    {
        static_assert(sizeof(Mem) == 32, "the record of caps_sa_hip_fm_mems");
        const uint64_t q = off.empty() ? 0 : off.size() - 1;
        mem_off.assign(static_cast<std::size_t>(q + 1), 0);
        const uint8_t* pat = reinterpret_cast<const uint8_t*>(patterns.data());
        check(caps_sa_hip_fm_mems(blob_.data(), blob_.size(), pat, off.data(), q, min_len, mem_off.data(), nullptr, 0, device_), "caps_sa_hip_fm_mems");
        mems.assign(static_cast<std::size_t>(mem_off[q]), Mem());
        if (!mems.empty())
            check(caps_sa_hip_fm_mems(blob_.data(), blob_.size(), pat, off.data(), q, min_len, mem_off.data(), mems.data(), mems.size(), device_),
                  "caps_sa_hip_fm_mems");
    }

    // Format version 2 in place (include/caps_sa_hip.h "FM-index: extract"): one row per t text positions behind the version-1
    // sections, derived from the SA samples.  An index without samples, t below sa_sample or no power of two up to 1024: thrown.
    void add_text_samples(uint32_t t = 32)
    {
        if (blob_.size() < 256) throw std::runtime_error("caps_sa_hip_fm_add_text_samples: not an FM-index blob");
        uint64_t h[32];
        std::memcpy(h, blob_.data(), sizeof h);
        uint64_t bytes = blob_.size();                       // (without SA samples: the library refuses below, with its reason)
        if (h[12] >= 1 && h[12] <= 1024)
            check(caps_sa_hip_fm_index_bytes_ex(h[2], static_cast<uint32_t>(h[12]), t, h[4] == 8 ? 8 : 4, &bytes), "caps_sa_hip_fm_index_bytes_ex");
        const std::size_t old = blob_.size();
        if (bytes > old) blob_.resize(static_cast<std::size_t>(bytes));
        const int rc = caps_sa_hip_fm_add_text_samples(blob_.data(), blob_.size(), t, device_);
        if (rc != CAPS_SA_OK) blob_.resize(old);
        check(rc, "caps_sa_hip_fm_add_text_samples");
        blob_.resize(static_cast<std::size_t>(bytes));
    }

    // 0: a version-1 blob (no extract)
    uint32_t text_sample() const
    {
        if (blob_.size() < 256) return 0;
        uint64_t h[32];
        std::memcpy(h, blob_.data(), sizeof h);
        return h[1] == 2 ? static_cast<uint32_t>(h[19]) : 0;
    }
    uint64_t n() const
    {
        uint64_t v = 0;
        if (blob_.size() >= 256) std::memcpy(&v, blob_.data() + 16, 8);
        return v;
    }

    // text[out_off[j] .. out_off[j + 1]) = T[start[j] .. start[j] + out_off[j + 1] - out_off[j]); out_off.size() = start.size() + 1
    void extract(const std::vector<uint64_t>& start, const std::vector<uint64_t>& out_off, std::string& text) const
    {
        const uint64_t q = start.size();
        if (out_off.size() != q + 1) throw std::runtime_error("FM_Index::extract: out_off must have one entry more than start");
        text.assign(static_cast<std::size_t>(out_off[q]), '\0');
        check(caps_sa_hip_fm_extract(blob_.data(), blob_.size(), start.data(), out_off.data(), q,
                                     text.empty() ? nullptr : reinterpret_cast<uint8_t*>(&text[0]), device_), "caps_sa_hip_fm_extract");
    }

    void save(const std::string& path) const
    {
        std::ofstream out(path, std::ios::binary);
        if (out) out.write(reinterpret_cast<const char*>(blob_.data()), static_cast<std::streamsize>(blob_.size()));
        if (!out) throw std::runtime_error(path + " : cannot write");
    }

    static FM_Index load(const std::string& path, int device = 0)
    {
        std::ifstream in(path, std::ios::binary | std::ios::ate);
        if (!in) throw std::runtime_error(path + " : cannot open");
        const std::streamsize size = in.tellg();
        FM_Index fm;
        fm.device_ = device;
        fm.blob_.resize(size > 0 ? static_cast<std::size_t>(size) : 0);
        in.seekg(0);
        if (size > 0 && !in.read(reinterpret_cast<char*>(fm.blob_.data()), size)) throw std::runtime_error(path + " : cannot read");
        return fm;
    }

private:
    static void check(int rc, const char* what)
    {
        if (rc != CAPS_SA_OK) throw std::runtime_error(std::string(what) + ": " + caps_sa_hip_last_error());
    }
    std::vector<uint8_t> blob_;
    int device_;
};

// LCE index over (SA, LCP) (include/caps_sa_hip.h "ISA and longest common extensions"; not in the reference): ISA, a copy of LCP and
// two tiers of range-minimum tables in one blob (data(), size()); lce() and range_min() answer batches on the GPU from the blob alone;
// save / load write and read exactly it.  Every error of the C ABI is thrown as std::runtime_error with its message.
class LCE_Index
{
public:
    LCE_Index() : device_(0) {}

    template <typename idx_t>
    static LCE_Index build(const idx_t* SA, const idx_t* LCP, uint64_t n, int device = 0)
    {
        static_assert(std::is_same<idx_t, uint32_t>::value || std::is_same<idx_t, uint64_t>::value, "uint32_t or uint64_t");
        LCE_Index x;
        x.device_ = device;
        uint64_t bytes = 0;
        check(caps_sa_hip_lce_index_bytes(n, (int)sizeof(idx_t), &bytes), "caps_sa_hip_lce_index_bytes");
        x.blob_.resize(static_cast<std::size_t>(bytes));
        if (sizeof(idx_t) == 4)
            check(caps_sa_hip_lce_build_u32(reinterpret_cast<const uint32_t*>(SA), reinterpret_cast<const uint32_t*>(LCP), n, x.blob_.data(), bytes, device),
                  "caps_sa_hip_lce_build_u32");
        else
            check(caps_sa_hip_lce_build_u64(reinterpret_cast<const uint64_t*>(SA), reinterpret_cast<const uint64_t*>(LCP), n, x.blob_.data(), bytes, device),
                  "caps_sa_hip_lce_build_u64");
        return x;
    }
    // from a constructed full-context Suffix_Array; a bounded-context one throws std::invalid_argument
    template <typename idx_t>
    static LCE_Index build(const Suffix_Array<idx_t>& sa)
    {
        if (!sa.full_context()) throw std::invalid_argument("LCE_Index::build: the index needs a full-context suffix array (max_context is set)");
        return build<idx_t>(sa.SA(), sa.LCP(), sa.n(), sa.device());
    }

    const uint8_t* data() const { return blob_.data(); }
    std::size_t size() const { return blob_.size(); }
    uint64_t n() const
    {
        uint64_t v = 0;
        if (blob_.size() >= 256) std::memcpy(&v, blob_.data() + 2 * 8, 8);      // header word 2
        return v;
    }

    // len[x] = the largest l such that T[i[x] .. i[x] + l) and T[j[x] .. j[x] + l) differ in at most `mismatches` (0 .. 1024) places
    std::vector<uint64_t> lce(const std::vector<uint64_t>& i, const std::vector<uint64_t>& j, uint64_t mismatches = 0) const
    {
        if (i.size() != j.size()) throw std::invalid_argument("LCE_Index::lce: two vectors of one size");
        std::vector<uint64_t> len(i.size());
        check(caps_sa_hip_lce(blob_.data(), blob_.size(), i.data(), j.data(), i.size(), mismatches, len.data(), device_), "caps_sa_hip_lce");
        return len;
    }
    // min[x] = min LCP[lo[x] .. hi[x]] over ranks, both ends inclusive, LCP[0] read as 0
    std::vector<uint64_t> range_min(const std::vector<uint64_t>& lo, const std::vector<uint64_t>& hi) const
    {
        if (lo.size() != hi.size()) throw std::invalid_argument("LCE_Index::range_min: two vectors of one size");
        std::vector<uint64_t> out(lo.size());
        check(caps_sa_hip_lce_range_min(blob_.data(), blob_.size(), lo.data(), hi.data(), lo.size(), out.data(), device_), "caps_sa_hip_lce_range_min");
        return out;
    }

    void save(const std::string& path) const
    {
        std::ofstream out(path, std::ios::binary);
        if (out) out.write(reinterpret_cast<const char*>(blob_.data()), static_cast<std::streamsize>(blob_.size()));
        if (!out) throw std::runtime_error(path + " : cannot write");
    }
    static LCE_Index load(const std::string& path, int device = 0)
    {
        std::ifstream in(path, std::ios::binary | std::ios::ate);
        if (!in) throw std::runtime_error(path + " : cannot open");
        const std::streamsize size = in.tellg();
        LCE_Index x;
        x.device_ = device;
        x.blob_.resize(size > 0 ? static_cast<std::size_t>(size) : 0);
        in.seekg(0);
        if (size > 0 && !in.read(reinterpret_cast<char*>(x.blob_.data()), size)) throw std::runtime_error(path + " : cannot read");
        return x;
    }

private:
    static void check(int rc, const char* what)
    {
        if (rc != CAPS_SA_OK) throw std::runtime_error(std::string(what) + ": " + caps_sa_hip_last_error());
    }
    std::vector<uint8_t> blob_;
    int device_;
};

}  // namespace CaPS_SA

#endif
