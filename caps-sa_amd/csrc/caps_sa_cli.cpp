// caps-sa_amd/csrc/caps_sa_cli.cpp -- command-line driver with the reference CLI's contract
// (reference src/main.cpp:43-93):
//
//     caps_sa <input_path> <output_path> [subproblem-count] [bounded-context] [--pretty-print] [--gpus N] [--bwt PATH]
//     caps_sa <input_path> <output_path> [subproblem-count] [--kmers K PATH [--min-count A] [--max-count B]] [--kmer-spectrum K PATH]
//     caps_sa <input_path> <output_path> [subproblem-count] [--lz77 PATH]
//     caps_sa <input_path> <output_path> [subproblem-count] [--lce-index PATH]
//     caps_sa --lce INDEX PAIRS [--mismatches K]
//     caps_sa <input_path> <output_path> [subproblem-count] [--raw] [--cross-mums SPLIT PATH] [--cross-mems SPLIT PATH [--max-occ C]] [--min-len L]
//     caps_sa --inverse-bwt IN.bwt OUT
//     caps_sa <input_path> <output_path> [subproblem-count] --fm-index PATH [--fm-sample S] [--fm-text-sample T]
//     caps_sa <input_path> <output_path> [subproblem-count] --raw [--bwt PATH] [--fm-index PATH [--fm-sample S]]
//     caps_sa --fm-search INDEX PATTERNS [--locate K]
//     caps_sa --fm-mems INDEX PATTERNS [--min-len L]
//     caps_sa --fm-from-bwt IN.bwt OUT.fm [--fm-sample S] [--fm-text-sample T]
//     caps_sa --fm-extract INDEX RANGES
//
// * --kmers K PATH [--min-count A] [--max-count B] (not in the reference; on the build line): after the SA / LCP output, the k-mer
//   table of the (remapped) text to PATH (include/caps_sa_hip.h "k-mers from SA and LCP"): one line "kmer<TAB>count" per distinct
//   K-mer with A <= count <= B (defaults: every count), in the library's byte order.  Refused with --raw (arbitrary bytes do not
//   make lines) and with a bounded context (its order is no suffix array), each with a message, before anything is written;
//   --min-count / --max-count without --kmers are refused;
// * --kmer-spectrum K PATH (not in the reference; on the build line): the multiplicity spectrum to PATH, one line "c number" for
//   c = 1 .. 1024: the distinct K-mers that occur c times (the last line: 1024 times or more).  Allowed with --raw; refused with a
//   bounded context;
// * --lz77 PATH (not in the reference; on the build line): after the SA / LCP output, the LZ77 factorization of the text as built
//   (remapped, or with --raw the file's own bytes) to PATH (include/caps_sa_hip.h "LPF and LZ77 from SA and LCP"): one line
//   "pos<TAB>len<TAB>src" per phrase in text order, the phrase being a copy of len bytes from position src (the two may overlap); a
//   literal is "pos<TAB>0<TAB>byte value in decimal", so the file alone decodes to the text.  Refused with a bounded context;
// * --lce-index PATH (not in the reference; on the build line): after the SA / LCP output, the LCE index of the two arrays to PATH
//   (include/caps_sa_hip.h "ISA and longest common extensions"): one blob that answers longest common extensions and range minima
//   over LCP without the text or the arrays.  Refused with a bounded context;
// * --lce INDEX PAIRS [--mismatches K] (not in the reference): one pair of text positions "i j" per line of PAIRS; per pair one line
//   on stdout, the length of the longest common extension of T[i ..) and T[j ..) with at most K (0 .. 1024, default 0) mismatches;
// * --docs FILE with --kmer-sharing K PATH and / or --coll-kmers K PATH [--min-docs A] [--max-docs B] (not in the reference; on the build
//   line): FILE holds one `start length` per line, up to 64 ascending, disjoint documents inside the text.  --kmer-sharing writes
//   `S<TAB>a<TAB>b<TAB>count` for a <= b (the k-mers documents a and b share), then `F<TAB>c<TAB>count` for c = 1 .. m (the k-mers in
//   exactly c documents); it works with --raw.  --coll-kmers writes `kmer<TAB>occ<TAB>docs as 16 hex digits` per k-mer in min-docs ..
//   max-docs documents and is refused with --raw for the reason --kmers is.  Either without --docs, a malformed or overlapping FILE,
//   --min-docs / --max-docs without --coll-kmers and a bounded context are refused before anything is written.
// * --cross-mums SPLIT PATH [--min-len L] and --cross-mems SPLIT PATH [--min-len L] [--max-occ C] (not in the reference; on the build
//   line): the text as built (remapped, or with --raw the file's own bytes) is A . sep . B with the separator at SPLIT - 1; after the
//   SA / LCP output, the maximal unique matches, or the maximal exact matches whose first L bytes occur at most C (2 .. 64, default
//   64) times, of at least L (default 1) bytes between the two sides to PATH (include/caps_sa_hip.h "MUMs and MEMs between two
//   texts"): one line "a<TAB>b<TAB>len" per record in record order, and on stderr one line with the summary.  A separator that occurs
//   nowhere else needs --raw (the remap leaves four letters).  One GPU; refused with a bounded context and with SPLIT > n, before
//   anything is written; --max-occ without --cross-mems is refused;
// * --raw (not in the reference; on the build line only): the text as given, no remap to {A,C,G,T} -- SA, LCP and --bwt are those of
//   the file's own bytes, and --fm-index PATH writes the wide format (include/caps_sa_hip.h "FM-index: the wide format") for 1 .. 256
//   distinct bytes.  --fm-search and --fm-mems tell a wide index by its magic and take the pattern lines as bytes, unremapped (a
//   line still ends at '\n' or "\r\n").  The wide format has no text samples and no extract: --raw with --fm-text-sample, and
//   --fm-extract on a wide index, are refused with a message that names the format, before anything is written.  Without --raw
//   nothing changes;
// * --fm-mems INDEX PATTERNS [--min-len L] (not in the reference): one pattern per line of PATTERNS, remapped like the text; per
//   line the number of its maximal exact matches of at least L (default 1) bytes against the text (include/caps_sa_hip.h "FM-index:
//   matching statistics"), then "start:length:count" for each by increasing end: start within the pattern, count = its occurrences
//   in the text.  Works on any index file, with or without samples.  Any other argument is refused;
// * --fm-text-sample T (not in the reference; with --fm-index PATH or --fm-from-bwt): the index is written in format version 2
//   (include/caps_sa_hip.h "FM-index: extract"), with the row of every T-th text position; T a power of two, S .. 1024;
// * --fm-extract INDEX RANGES (not in the reference): one "start length" pair per line of RANGES; per line the text
//   T[start .. start + length) of the (remapped) text, from the index alone.  A malformed line, a range past n, an index of format
//   version 1 and any other argument are refused before anything is printed;
// * --fm-from-bwt IN.bwt OUT.fm [--fm-sample S] (not in the reference): the FM-index WITH its SA samples from a file that --bwt
//   wrote and nothing else (include/caps_sa_hip.h "FM-index from the BWT alone"): byte for byte what --fm-index writes for the
//   same text.  IN is read and checked as --inverse-bwt does; 32-bit indices for n <= UINT32_MAX; every refusal comes before OUT
//   is opened, OUT is written only after the build has succeeded.  Any other argument is refused;
// * --fm-index PATH [--fm-sample S] (not in the reference): also write the FM-index of the (remapped) text to PATH (the blob of
//   include/caps_sa_hip.h "FM-index", SA samples every S = 32 text positions; S a power of two, 1 .. 1024).  One GPU, no bounded
//   context, like --bwt: refused before any file is opened;
// * --fm-search INDEX PATTERNS [--locate K] (not in the reference): one pattern per line of PATTERNS, remapped like the text;
//   per line the count, and with --locate K up to K positions in suffix-array order.  Any other argument is refused;
// * --inverse-bwt IN.bwt OUT (not in the reference): the text back from a file that --bwt wrote (u64 n, u64 primary, n bytes):
//   its n bytes to OUT, written only after the inverse has succeeded.  An unreadable IN, a size other than 16 + n, primary >= n
//   and any other argument are refused before OUT is opened;
// * --gpus N (not in the reference): shard the build over HIP devices 0 .. N-1;
// * --bwt PATH (not in the reference): also write the Burrows-Wheeler transform of the (remapped) text to PATH after the SA / LCP
//   output: u64 n, u64 primary, n bytes, native endianness (include/caps_sa_hip.h has the definition).  One GPU, no bounded
//   context: both are refused before any file is opened;
// * bounded-context (main.cpp:57): 0 or >= the text length = the suffix array; a smaller bound takes the reference's own
//   sequence of merges (csrc/bounded.h: its output depends on them; a compatibility mode, seconds instead of milliseconds);
// * every input byte is remapped to {A,C,G,T} with lookup[(toupper(c) & 0x6) >> 1],
//   lookup = {A,C,T,G} (main.cpp:61-70) -- FASTA headers and newlines are kept and remapped;
// * n = file size; n <= UINT32_MAX selects 32-bit indices, else 64-bit (main.cpp:76-87);
// * output = Suffix_Array::dump format (u64 n, SA, LCP; src/Suffix_Array.cpp:497-509), or,
//   with --pretty-print (advertised at main.cpp:49 but never wired up there), the text
//   form of main.cpp:32-40: one line of SA values, one line of LCP values.
#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <string>
#include <thread>
#include <vector>

#include <sys/stat.h>

#include "Suffix_Array.hpp"

// A driver that compiles this file over a renamed C ABI (#define caps_sa_hip_build_multi_u32 ...) and was written before the k-mer
// entry points existed has no twin for them to link against: it gets the CLI without --kmers / --kmer-spectrum (both refused).
#if defined(caps_sa_hip_build_multi_u32) && !defined(caps_sa_hip_kmers_u32)
#define CAPS_CLI_NO_KMERS 1
#endif
// ... and the same for a driver that predates the LZ77 entry points: the CLI without --lz77.
#if defined(caps_sa_hip_build_multi_u32) && !defined(caps_sa_hip_lz77_u32)
#define CAPS_CLI_NO_LZ 1
#endif
// ... and for one that predates the LCE entry points: the CLI without --lce-index and --lce.
#if defined(caps_sa_hip_build_multi_u32) && !defined(caps_sa_hip_lce_build_u32)
#define CAPS_CLI_NO_LCE 1
#endif

// ... and for one that predates the MUM / MEM entry points: the CLI without --cross-mums and --cross-mems.
#if defined(caps_sa_hip_build_multi_u32) && !defined(caps_sa_hip_cross_mums_u32)
#define CAPS_CLI_NO_CROSS 1
#endif

// ... and for one that predates the collection k-mer entry points: the CLI without --kmer-sharing and --coll-kmers.
#if defined(caps_sa_hip_build_multi_u32) && !defined(caps_sa_hip_coll_kmers_u32)
#define CAPS_CLI_NO_COLL 1
#endif

static bool read_input(const std::string& path, std::string& text)
{
    std::ifstream in(path, std::ios::binary | std::ios::ate);
    if (!in) { std::cerr << path << " : cannot open\n"; return false; }
    const std::streamsize size = in.tellg();
    in.seekg(0);
    text.resize(static_cast<size_t>(size));
    in.read(&text[0], size);
    return static_cast<bool>(in) || size == 0;
}

// positional numeric argument: digits only, fits size_t
static bool parse_count(const std::string& s, size_t& out)
{
    if (s.empty() || s.size() > 19) return false;
    size_t v = 0;
    for (char c : s) {
        if (c < '0' || c > '9') return false;
        v = v * 10 + static_cast<size_t>(c - '0');
    }
    out = v;
    return true;
}

// what --kmers / --kmer-spectrum ask for (k = 0: not asked for)
struct KmerJob {
    size_t k = 0, min_count = 1, max_count = 0, spectrum_k = 0;
    std::string path, spectrum_path;
};

// what --cross-mums / --cross-mems ask for (an empty path: not asked for)
struct CrossJob {
    size_t mums_split = 0, mems_split = 0, min_len = 1, max_occ = 64;
    std::string mums_path, mems_path;
    bool any() const { return !mums_path.empty() || !mems_path.empty(); }
};

// what --docs / --kmer-sharing / --coll-kmers ask for (k = 0: not asked for)
struct CollJob {
    std::vector<std::pair<uint64_t, uint64_t>> docs;
    size_t sharing_k = 0, kmers_k = 0, min_docs = 1, max_docs = 0;
    std::string sharing_path, kmers_path;
    bool any() const { return sharing_k || kmers_k; }
};

// a --docs file: one `start length` per line, 1 .. 64 lines, ascending and disjoint inside a text of n bytes
static bool read_docs(const std::string& path, size_t n, std::vector<std::pair<uint64_t, uint64_t>>& docs, std::string& why)
{
    std::string lines;
    {
        std::ifstream in(path, std::ios::binary);
        if (!in) { why = "cannot open " + path; return false; }
        lines.assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
    }
    size_t prev_end = 0;
    for (size_t a = 0; a < lines.size();) {
        size_t b = lines.find('\n', a);
        if (b == std::string::npos) b = lines.size();
        std::string line = lines.substr(a, b - a);
        a = b + 1;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        const size_t sp = line.find_first_of(" \t");
        size_t start = 0, len = 0;
        if (sp == std::string::npos || !parse_count(line.substr(0, sp), start) || !parse_count(line.substr(line.find_first_not_of(" \t", sp)), len)) {
            why = "line " + std::to_string(docs.size() + 1) + " is not `start length`: " + line;
            return false;
        }
        if (len > n || start > n - len) { why = "document " + std::to_string(docs.size()) + " passes the end of the text (n = " + std::to_string(n) + ")"; return false; }
        if (start < prev_end) { why = "document " + std::to_string(docs.size()) + " overlaps or precedes the one before it"; return false; }
        prev_end = start + len;
        docs.emplace_back(start, len);
        if (docs.size() > 64) { why = "more than 64 documents"; return false; }
    }
    if (docs.empty()) { why = "no document in " + path; return false; }
    return true;
}

template <typename idx_t>
static int run(const std::string& text, const std::string& out_path, size_t p, size_t ctx, bool pretty, const std::vector<int>& devices,
               const std::string& bwt_path, const std::string& fm_path = std::string(), uint32_t fm_sample = 32, uint32_t fm_text_sample = 0, bool raw = false,
               const KmerJob& km = KmerJob(), const std::string& lz_path = std::string(), const std::string& lce_path = std::string(),
               const CrossJob& cross = CrossJob(), const CollJob& coll = CollJob())
{
    if (p > std::numeric_limits<idx_t>::max()) { std::cerr << "subproblem-count does not fit the index type\n"; return EXIT_FAILURE; }
    // the bounded-context mode replays the reference's merge history, one GPU thread per merge node -- the top levels
    // of its trees are sequential merges of O(n) elements (9.5 s at 64 Mi chars; the reference itself: 67 s on one thread there).
    // Say so before a genome-sized run looks like a hang.
    if (ctx != 0 && ctx < text.size() && text.size() >= (size_t(64) << 20))
        std::cerr << "bounded-context " << ctx << ": compatibility mode (csrc/bounded.h), about " << (text.size() >> 20) * 0.15
                  << " seconds for " << (text.size() >> 20) << " Mi chars; the unbounded construction takes milliseconds.\n";
    CaPS_SA::Suffix_Array<idx_t> suf_arr(text.c_str(), static_cast<idx_t>(text.size()), static_cast<idx_t>(p),
                                         static_cast<idx_t>(ctx >= text.size() ? 0 : ctx), devices);
    if (bwt_path.empty() && fm_path.empty() && !cross.any()) suf_arr.construct();
    else suf_arr.construct_bwt();
    const caps_sa_stats& st = suf_arr.stats();
    std::cerr << "Constructed the suffix array. Device time: " << st.ms_total / 1e3 << " seconds (h2d "
              << st.ms_h2d / 1e3 << ", d2h " << st.ms_d2h / 1e3 << "); subproblems " << st.p_eff << ", "
              << st.bits_per_char << " bits/char, " << devices.size() << " GPU(s).\n";
    std::ofstream output(out_path, std::ios::binary);           // only now: a failed build leaves no empty file behind
    if (!output) { std::cerr << out_path << " : cannot open for writing\n"; return EXIT_FAILURE; }
    if (pretty) {
        const size_t n = suf_arr.n();
        for (size_t i = 0; i < n; ++i) output << suf_arr.SA()[i] << " \n"[i == n - 1];
        for (size_t i = 0; i < n; ++i) output << suf_arr.LCP()[i] << " \n"[i == n - 1];
    } else
        suf_arr.dump(output);
    if (!output) return EXIT_FAILURE;
    if (!bwt_path.empty()) {
        std::ofstream bwt(bwt_path, std::ios::binary);
        if (!bwt) { std::cerr << bwt_path << " : cannot open for writing\n"; return EXIT_FAILURE; }
        const uint64_t n = suf_arr.n(), primary = suf_arr.primary();
        bwt.write(reinterpret_cast<const char*>(&n), sizeof n);
        bwt.write(reinterpret_cast<const char*>(&primary), sizeof primary);
        bwt.write(reinterpret_cast<const char*>(suf_arr.BWT()), static_cast<std::streamsize>(n));
        if (!bwt) return EXIT_FAILURE;
    }
    if (!fm_path.empty()) {
        CaPS_SA::FM_Index fm = raw ? CaPS_SA::FM_Index::build_wide<idx_t>(suf_arr.BWT(), suf_arr.n(), suf_arr.primary(), suf_arr.SA(), fm_sample)
                                   : CaPS_SA::FM_Index::build<idx_t>(suf_arr.BWT(), suf_arr.n(), suf_arr.primary(), suf_arr.SA(), fm_sample);
        if (fm_text_sample) fm.add_text_samples(fm_text_sample);
        fm.save(fm_path);
        std::cerr << "FM-index: " << fm.size() << " bytes";
        if (raw) std::cerr << " (wide format, " << fm.sigma() << " letters)";
        std::cerr << ", SA samples every " << fm_sample << " positions";
        if (fm_text_sample) std::cerr << ", text samples every " << fm_text_sample;
        std::cerr << ".\n";
    }
#ifndef CAPS_CLI_NO_KMERS
    if (km.k) {
        const auto table = suf_arr.kmers(km.k, km.min_count, km.max_count);
        std::ofstream out(km.path, std::ios::binary);
        if (!out) { std::cerr << km.path << " : cannot open for writing\n"; return EXIT_FAILURE; }
        for (const auto& r : table) {
            out.write(text.data() + r.pos, static_cast<std::streamsize>(km.k));
            out << '\t' << r.count << '\n';
        }
        if (!out) return EXIT_FAILURE;
        std::cerr << "k-mers: " << table.size() << " distinct " << km.k << "-mers written.\n";
    }
    if (km.spectrum_k) {
        const std::vector<uint64_t> hist = suf_arr.kmer_spectrum(km.spectrum_k, 1024);
        std::ofstream out(km.spectrum_path, std::ios::binary);
        if (!out) { std::cerr << km.spectrum_path << " : cannot open for writing\n"; return EXIT_FAILURE; }
        for (size_t c = 1; c <= 1024; ++c) out << c << ' ' << hist[c] << '\n';
        if (!out) return EXIT_FAILURE;
    }
#endif
#ifndef CAPS_CLI_NO_LZ
    if (!lz_path.empty()) {
        const auto parse = suf_arr.lz77();
        std::ofstream out(lz_path, std::ios::binary);
        if (!out) { std::cerr << lz_path << " : cannot open for writing\n"; return EXIT_FAILURE; }
        for (const auto& ph : parse) {
            if (ph.src == suf_arr.literal) out << ph.pos << "\t0\t" << static_cast<unsigned>(static_cast<unsigned char>(text[ph.pos])) << '\n';
            else out << ph.pos << '\t' << ph.len << '\t' << ph.src << '\n';
        }
        if (!out) return EXIT_FAILURE;
        std::cerr << "LZ77: " << parse.size() << " phrases written.\n";
    }
#endif
#ifndef CAPS_CLI_NO_LCE
    if (!lce_path.empty()) {
        const CaPS_SA::LCE_Index x = CaPS_SA::LCE_Index::build(suf_arr);
        x.save(lce_path);
        std::cerr << "LCE index: " << x.size() << " bytes written.\n";
    }
#endif
#ifndef CAPS_CLI_NO_CROSS
    for (int mems = 0; mems < 2; ++mems) {
        const std::string& path = mems ? cross.mems_path : cross.mums_path;
        if (path.empty()) continue;
        typename CaPS_SA::Suffix_Array<idx_t>::Cross_Summary s{};
        const auto rec = mems ? suf_arr.cross_mems(cross.mems_split, cross.min_len, static_cast<uint32_t>(cross.max_occ), &s)
                              : suf_arr.cross_mums(cross.mums_split, cross.min_len, &s);
        std::ofstream out(path, std::ios::binary);
        if (!out) { std::cerr << path << " : cannot open for writing\n"; return EXIT_FAILURE; }
        for (const auto& r : rec) out << r.a << '\t' << r.b << '\t' << r.len << '\n';
        if (!out) return EXIT_FAILURE;
        std::cerr << (mems ? "cross-mems: " : "cross-mums: ") << s.records << " records, " << s.skipped_runs << " skipped runs, longest common substring "
                  << s.lcs_len << " at " << s.lcs_a << " and " << s.lcs_b << ".\n";
    }
#endif
#ifndef CAPS_CLI_NO_COLL
    if (coll.sharing_k) {
        std::vector<uint64_t> freq, shared;
        suf_arr.kmer_sharing(coll.sharing_k, coll.docs, freq, shared);
        const size_t m = coll.docs.size();
        std::ofstream out(coll.sharing_path, std::ios::binary);
        if (!out) { std::cerr << coll.sharing_path << " : cannot open for writing\n"; return EXIT_FAILURE; }
        for (size_t a = 0; a < m; ++a)
            for (size_t b = a; b < m; ++b) out << "S\t" << a << '\t' << b << '\t' << shared[a * m + b] << '\n';
        uint64_t total = 0;
        for (size_t c = 1; c <= m; ++c) { out << "F\t" << c << '\t' << freq[c] << '\n'; total += freq[c]; }
        if (!out) return EXIT_FAILURE;
        std::cerr << "k-mer sharing: " << total << " distinct " << coll.sharing_k << "-mers in " << m << " documents, " << freq[m] << " in all of them.\n";
    }
    if (coll.kmers_k) {
        const auto table = suf_arr.collection_kmers(coll.kmers_k, coll.docs, coll.min_docs, coll.max_docs);
        std::ofstream out(coll.kmers_path, std::ios::binary);
        if (!out) { std::cerr << coll.kmers_path << " : cannot open for writing\n"; return EXIT_FAILURE; }
        char hex[17];
        for (const auto& r : table) {
            out.write(text.data() + suf_arr.SA()[r.first], static_cast<std::streamsize>(coll.kmers_k));
            std::snprintf(hex, sizeof hex, "%016llx", static_cast<unsigned long long>(r.docs));
            out << '\t' << r.occ << '\t' << hex << '\n';
        }
        if (!out) return EXIT_FAILURE;
        std::cerr << "collection k-mers: " << table.size() << " " << coll.kmers_k << "-mers written.\n";
    }
#endif
    return 0;
}

// the lines of a PATTERNS file, concatenated: remapped like the text for an index of the remapped text, as bytes for a wide index
// (which --raw wrote over the text's own bytes)
static void read_patterns(const std::string& lines, bool as_bytes, std::string& pats, std::vector<uint64_t>& off)
{
    static const char lookup[4] = {'A', 'C', 'T', 'G'};
    off.assign(1, 0);
    for (size_t a = 0; a < lines.size();) {
        size_t b = lines.find('\n', a);
        if (b == std::string::npos) b = lines.size();
        size_t e = b;
        if (e > a && lines[e - 1] == '\r') --e;
        if (as_bytes) pats.append(lines, a, e - a);
        else
            for (size_t j = a; j < e; ++j) pats.push_back(lookup[(std::toupper(static_cast<unsigned char>(lines[j])) & 0x6) >> 1]);
        off.push_back(pats.size());
        a = b + 1;
    }
}

// caps_sa --fm-search INDEX PATTERNS [--locate K]: args = everything after the program name
static int fm_search_main(const std::vector<std::string>& args)
{
    const char* usage = "--fm-search: usage: caps_sa --fm-search INDEX PATTERNS [--locate K] (no other option or argument)\n";
    if (args.size() < 3 || args[0] != "--fm-search" || (args.size() != 3 && args.size() != 5)) { std::cerr << usage; return EXIT_FAILURE; }
    size_t k = 0;
    const bool locate = args.size() == 5;
    if (locate && (args[3] != "--locate" || !parse_count(args[4], k) || k < 1)) { std::cerr << usage; return EXIT_FAILURE; }
    if (args[1].compare(0, 2, "--") == 0 || args[2].compare(0, 2, "--") == 0) { std::cerr << usage; return EXIT_FAILURE; }
    std::string lines;
    if (!read_input(args[2], lines)) return EXIT_FAILURE;
    try {
        const CaPS_SA::FM_Index fm = CaPS_SA::FM_Index::load(args[1]);
        std::string pats;
        std::vector<uint64_t> off;
        read_patterns(lines, fm.wide(), pats, off);
        std::vector<uint64_t> first, cnt, out_off, pos;
        fm.count(pats, off, first, cnt);
        if (locate) fm.locate(first, cnt, k, out_off, pos);
        for (size_t j = 0; j + 1 < off.size(); ++j) {
            std::cout << cnt[j];
            if (locate)
                for (uint64_t t = out_off[j]; t < out_off[j + 1]; ++t) std::cout << ' ' << pos[t];
            std::cout << '\n';
        }
    } catch (const std::exception& e) {
        std::cerr << e.what() << "\n";
        return EXIT_FAILURE;
    }
    return 0;
}

// caps_sa --fm-mems INDEX PATTERNS [--min-len L]: args = everything after the program name
static int fm_mems_main(const std::vector<std::string>& args)
{
    const char* usage = "--fm-mems: usage: caps_sa --fm-mems INDEX PATTERNS [--min-len L] (no other option or argument)\n";
    if (args.size() < 3 || args[0] != "--fm-mems" || (args.size() != 3 && args.size() != 5)) { std::cerr << usage; return EXIT_FAILURE; }
    size_t min_len = 1;
    if (args.size() == 5 && (args[3] != "--min-len" || !parse_count(args[4], min_len) || min_len < 1 || min_len > 0xFFFFFFFFull)) {
        std::cerr << usage;
        return EXIT_FAILURE;
    }
    if (args[1].compare(0, 2, "--") == 0 || args[2].compare(0, 2, "--") == 0) { std::cerr << usage; return EXIT_FAILURE; }
    std::string lines;
    if (!read_input(args[2], lines)) return EXIT_FAILURE;
    try {
        const CaPS_SA::FM_Index fm = CaPS_SA::FM_Index::load(args[1]);
        std::string pats;
        std::vector<uint64_t> off;
        read_patterns(lines, fm.wide(), pats, off);
        std::vector<uint64_t> mem_off;
        std::vector<CaPS_SA::FM_Index::Mem> mems;
        fm.mems(pats, off, static_cast<uint32_t>(min_len), mem_off, mems);
        for (size_t j = 0; j + 1 < off.size(); ++j) {
            std::cout << mem_off[j + 1] - mem_off[j];
            for (uint64_t t = mem_off[j]; t < mem_off[j + 1]; ++t) std::cout << ' ' << mems[t].start << ':' << mems[t].length << ':' << mems[t].count;
            std::cout << '\n';
        }
    } catch (const std::exception& e) {
        std::cerr << e.what() << "\n";
        return EXIT_FAILURE;
    }
    return 0;
}

// a file that --bwt wrote (u64 n, u64 primary, n bytes) into data; false with the reason on stderr, prefixed by the option's name
static bool read_bwt_file(const char* opt, const std::string& in_path, std::string& data, uint64_t& n, uint64_t& primary)
{
    {
        std::ifstream in(in_path, std::ios::binary | std::ios::ate);
        if (!in) { std::cerr << opt << ": " << in_path << " : cannot open\n"; return false; }
        const std::streamsize size = in.tellg();
        if (size < 0) { std::cerr << opt << ": " << in_path << " : cannot read\n"; return false; }
        in.seekg(0);
        data.resize(static_cast<size_t>(size));
        if (size && !in.read(&data[0], size)) { std::cerr << opt << ": " << in_path << " : cannot read\n"; return false; }
    }
    if (data.size() < 16) {
        std::cerr << opt << ": " << in_path << " is " << data.size() << " bytes, shorter than its 16-byte header (u64 n, u64 primary)\n";
        return false;
    }
    std::memcpy(&n, data.data(), 8);
    std::memcpy(&primary, data.data() + 8, 8);
    if (data.size() - 16 != n) {
        std::cerr << opt << ": " << in_path << " holds " << data.size() - 16 << " bytes after its header, its n says " << n << "\n";
        return false;
    }
    if (n && primary >= n) { std::cerr << opt << ": primary " << primary << " >= n " << n << "\n"; return false; }
    return true;
}

// caps_sa --fm-from-bwt IN OUT [--fm-sample S]: args = everything after the program name
static int fm_from_bwt_main(const std::vector<std::string>& args)
{
    const char* usage = "--fm-from-bwt: usage: caps_sa --fm-from-bwt IN.bwt OUT.fm [--fm-sample S] [--fm-text-sample T] (no other option or argument)\n";
    if ((args.size() != 3 && args.size() != 5 && args.size() != 7) || args[0] != "--fm-from-bwt" || args[1].compare(0, 2, "--") == 0 ||
        args[2].compare(0, 2, "--") == 0) {
        std::cerr << usage;
        return EXIT_FAILURE;
    }
    size_t sample = 32, text_sample = 0;
    bool have_sample = false, have_text = false;
    for (size_t i = 3; i < args.size(); i += 2) {            // each option once, with its value
        if (args[i] == "--fm-sample" && !have_sample) have_sample = true;
        else if (args[i] == "--fm-text-sample" && !have_text) have_text = true;
        else { std::cerr << usage; return EXIT_FAILURE; }
    }
    for (size_t i = 3; i < args.size(); i += 2) {
        if (args[i] == "--fm-sample" && (!parse_count(args[i + 1], sample) || sample < 1 || sample > 1024 || (sample & (sample - 1)))) {
            std::cerr << "--fm-sample: a power of two in 1 .. 1024, please\n";
            return EXIT_FAILURE;
        }
        if (args[i] == "--fm-text-sample" && (!parse_count(args[i + 1], text_sample) || text_sample < 1 || text_sample > 1024 || (text_sample & (text_sample - 1)))) {
            std::cerr << "--fm-text-sample: a power of two in the --fm-sample distance .. 1024, please\n";
            return EXIT_FAILURE;
        }
    }
    if (have_text && text_sample < sample) {
        std::cerr << "--fm-text-sample: a power of two in the --fm-sample distance .. 1024, please (--fm-sample is " << sample << ")\n";
        return EXIT_FAILURE;
    }
    std::string data;
    uint64_t n = 0, primary = 0;
    if (!read_bwt_file("--fm-from-bwt", args[1], data, n, primary)) return EXIT_FAILURE;
    try {
        CaPS_SA::FM_Index fm = CaPS_SA::FM_Index::build_from_bwt(reinterpret_cast<const uint8_t*>(data.data() + 16), n, primary,
                                                                 static_cast<uint32_t>(sample));
        if (have_text) fm.add_text_samples(static_cast<uint32_t>(text_sample));
        fm.save(args[2]);
        std::cerr << "FM-index: " << fm.size() << " bytes, SA samples every " << sample << " positions";
        if (have_text) std::cerr << ", text samples every " << text_sample;
        std::cerr << ".\n";
    } catch (const std::exception& e) {
        std::cerr << e.what() << "\n";
        return EXIT_FAILURE;
    }
    return 0;
}

// caps_sa --fm-extract INDEX RANGES: args = everything after the program name
static int fm_extract_main(const std::vector<std::string>& args)
{
    const char* usage = "--fm-extract: usage: caps_sa --fm-extract INDEX RANGES (no other option or argument)\n";
    if (args.size() != 3 || args[0] != "--fm-extract" || args[1].compare(0, 2, "--") == 0 || args[2].compare(0, 2, "--") == 0) {
        std::cerr << usage;
        return EXIT_FAILURE;
    }
    std::string lines;
    if (!read_input(args[2], lines)) { std::cerr << "--fm-extract: no ranges read\n"; return EXIT_FAILURE; }
    std::vector<uint64_t> start, off(1, 0);
    size_t line_no = 0;
    for (size_t a = 0; a < lines.size();) {                  // "start length", one blank or tab between them, nothing else
        size_t b = lines.find('\n', a);
        if (b == std::string::npos) b = lines.size();
        size_t e = b;
        if (e > a && lines[e - 1] == '\r') --e;
        ++line_no;
        const std::string line = lines.substr(a, e - a);
        const size_t sp = line.find_first_of(" \t");
        size_t s = 0, len = 0;
        if (sp == std::string::npos || !parse_count(line.substr(0, sp), s) || !parse_count(line.substr(sp + 1), len)) {
            std::cerr << "--fm-extract: " << args[2] << " line " << line_no << ": expected \"start length\", two numbers\n";
            return EXIT_FAILURE;
        }
        start.push_back(s);
        off.push_back(off.back() + len);
        a = b + 1;
    }
    try {
        const CaPS_SA::FM_Index fm = CaPS_SA::FM_Index::load(args[1]);
        if (fm.wide()) {
            std::cerr << "--fm-extract: " << args[1] << " is a wide FM-index (\"CAPSFMW1\", written by --raw --fm-index): extract is not built for the wide format\n";
            return EXIT_FAILURE;
        }
        if (fm.size() < 256 || std::memcmp(fm.data(), "CAPSFMI1", 8) != 0) {
            std::cerr << "--fm-extract: " << args[1] << " is not an FM-index of this library\n";
            return EXIT_FAILURE;
        }
        if (fm.text_sample() == 0) {
            std::cerr << "--fm-extract: " << args[1] << " has no text-position samples (format version 1): build it with --fm-text-sample T\n";
            return EXIT_FAILURE;
        }
        for (size_t j = 0; j < start.size(); ++j)
            if (start[j] > fm.n() || off[j + 1] - off[j] > fm.n() - start[j]) {
                std::cerr << "--fm-extract: " << args[2] << " line " << j + 1 << ": the range ends past the text (n = " << fm.n() << ")\n";
                return EXIT_FAILURE;
            }
        std::string text;
        fm.extract(start, off, text);
        for (size_t j = 0; j < start.size(); ++j) {
            std::cout.write(text.data() + off[j], static_cast<std::streamsize>(off[j + 1] - off[j]));
            std::cout << '\n';
        }
    } catch (const std::exception& e) {
        std::cerr << "--fm-extract: " << e.what() << "\n";
        return EXIT_FAILURE;
    }
    return 0;
}

// caps_sa --lce INDEX PAIRS [--mismatches K]: args = everything after the program name
static int lce_main(const std::vector<std::string>& args)
{
#ifdef CAPS_CLI_NO_LCE
    std::cerr << "--lce: not built into this driver\n";
    return EXIT_FAILURE;
#else
    const char* usage = "--lce: usage: caps_sa --lce INDEX PAIRS [--mismatches K] (no other option or argument)\n";
    if (args.size() < 3 || args[0] != "--lce" || (args.size() != 3 && args.size() != 5) || args[1].compare(0, 2, "--") == 0 ||
        args[2].compare(0, 2, "--") == 0) {
        std::cerr << usage;
        return EXIT_FAILURE;
    }
    size_t k = 0;
    if (args.size() == 5 && (args[3] != "--mismatches" || !parse_count(args[4], k) || k > 1024)) {
        std::cerr << "--mismatches: needs a number in 0 .. 1024\n" << usage;
        return EXIT_FAILURE;
    }
    std::string lines;
    if (!read_input(args[2], lines)) { std::cerr << "--lce: no pairs read\n"; return EXIT_FAILURE; }
    std::vector<uint64_t> I, J;
    size_t line_no = 0;
    for (size_t a = 0; a < lines.size();) {                  // "i j", one blank or tab between them, nothing else
        size_t b = lines.find('\n', a);
        if (b == std::string::npos) b = lines.size();
        size_t e = b;
        if (e > a && lines[e - 1] == '\r') --e;
        ++line_no;
        const std::string line = lines.substr(a, e - a);
        const size_t sp = line.find_first_of(" \t");
        size_t i = 0, j = 0;
        if (sp == std::string::npos || !parse_count(line.substr(0, sp), i) || !parse_count(line.substr(sp + 1), j)) {
            std::cerr << "--lce: " << args[2] << " line " << line_no << ": expected \"i j\", two numbers\n";
            return EXIT_FAILURE;
        }
        I.push_back(i);
        J.push_back(j);
        a = b + 1;
    }
    try {
        const CaPS_SA::LCE_Index x = CaPS_SA::LCE_Index::load(args[1]);
        if (x.size() < 256 || std::memcmp(x.data(), "CAPSLCE1", 8) != 0) {
            std::cerr << "--lce: " << args[1] << " is not an LCE index of this library\n";
            return EXIT_FAILURE;
        }
        for (size_t q = 0; q < I.size(); ++q)
            if (I[q] >= x.n() || J[q] >= x.n()) {
                std::cerr << "--lce: " << args[2] << " line " << q + 1 << ": a position is past the text (n = " << x.n() << ")\n";
                return EXIT_FAILURE;
            }
        const std::vector<uint64_t> len = x.lce(I, J, k);
        for (size_t q = 0; q < len.size(); ++q) std::cout << len[q] << '\n';
    } catch (const std::exception& e) {
        std::cerr << "--lce: " << e.what() << "\n";
        return EXIT_FAILURE;
    }
    return 0;
#endif
}

// caps_sa --inverse-bwt IN OUT: args = everything after the program name
static int inverse_bwt_main(const std::vector<std::string>& args)
{
    if (args.size() != 3 || args[0] != "--inverse-bwt") {
        std::cerr << "--inverse-bwt: usage: caps_sa --inverse-bwt IN.bwt OUT (no other option or argument)\n";
        return EXIT_FAILURE;
    }
    const std::string& in_path = args[1];
    const std::string& out_path = args[2];
    std::string data;
    uint64_t n = 0, primary = 0;
    if (!read_bwt_file("--inverse-bwt", in_path, data, n, primary)) return EXIT_FAILURE;
    std::string text(static_cast<size_t>(n), '\0');
    try {
        CaPS_SA::inverse_bwt(reinterpret_cast<const uint8_t*>(data.data() + 16), n, primary, n ? &text[0] : nullptr);
    } catch (const std::exception& e) {
        std::cerr << e.what() << "\n";
        return EXIT_FAILURE;
    }
    std::ofstream out(out_path, std::ios::binary);
    if (!out) { std::cerr << out_path << " : cannot open for writing\n"; return EXIT_FAILURE; }
    out.write(text.data(), static_cast<std::streamsize>(n));
    return out ? 0 : EXIT_FAILURE;
}

int main(int argc, char* argv[])
{
    for (int i = 1; i < argc; ++i)
        if (std::strcmp(argv[i], "--inverse-bwt") == 0) return inverse_bwt_main(std::vector<std::string>(argv + 1, argv + argc));
    for (int i = 1; i < argc; ++i)
        if (std::strcmp(argv[i], "--fm-search") == 0) return fm_search_main(std::vector<std::string>(argv + 1, argv + argc));
    for (int i = 1; i < argc; ++i)
        if (std::strcmp(argv[i], "--fm-mems") == 0) return fm_mems_main(std::vector<std::string>(argv + 1, argv + argc));
    for (int i = 1; i < argc; ++i)
        if (std::strcmp(argv[i], "--fm-from-bwt") == 0) return fm_from_bwt_main(std::vector<std::string>(argv + 1, argv + argc));
    for (int i = 1; i < argc; ++i)
        if (std::strcmp(argv[i], "--fm-extract") == 0) return fm_extract_main(std::vector<std::string>(argv + 1, argv + argc));
    for (int i = 1; i < argc; ++i)
        if (std::strcmp(argv[i], "--lce") == 0) return lce_main(std::vector<std::string>(argv + 1, argv + argc));
    std::vector<std::string> pos;
    std::string lce_path;                                  // --lce-index (empty: not asked for)
    bool lce = false;
    bool pretty = false, bwt = false, fm = false, fm_sample_given = false, fm_text_given = false, raw = false;
    size_t gpus = 1, fm_sample = 32, fm_text_sample = 0;
    std::string bwt_path, fm_path;
    KmerJob km;
    std::string lz_path;                                   // --lz77 (empty: not asked for)
    bool kmers = false, spectrum = false, min_count_given = false, max_count_given = false, lz = false;
    CrossJob cross;                                        // --cross-mums / --cross-mems
    bool min_len_given = false, max_occ_given = false;
    CollJob coll;                                          // --docs / --kmer-sharing / --coll-kmers
    std::string docs_path;
    bool docs_given = false, min_docs_given = false, max_docs_given = false;
    for (int i = 1; i < argc; ++i) {
        if (std::strcmp(argv[i], "--pretty-print") == 0) pretty = true;
        else if (std::strcmp(argv[i], "--docs") == 0) {
            if (docs_given) { std::cerr << "--docs: given twice\n"; return EXIT_FAILURE; }
            if (i + 1 >= argc || std::strncmp(argv[i + 1], "--", 2) == 0 || !argv[i + 1][0]) { std::cerr << "--docs: usage: --docs FILE\n"; return EXIT_FAILURE; }
            docs_given = true;
            docs_path = argv[++i];
        }
        else if (std::strcmp(argv[i], "--kmer-sharing") == 0 || std::strcmp(argv[i], "--coll-kmers") == 0) {
            const bool table = std::strcmp(argv[i], "--coll-kmers") == 0;
            const char* opt = argv[i];
            size_t k = 0;
            if ((table ? coll.kmers_k : coll.sharing_k)) { std::cerr << opt << ": given twice\n"; return EXIT_FAILURE; }
            if (i + 2 >= argc || !parse_count(argv[i + 1], k) || k < 1 || std::strncmp(argv[i + 2], "--", 2) == 0 || !argv[i + 2][0]) {
                std::cerr << opt << ": usage: " << opt << " K PATH (K >= 1)\n";
                return EXIT_FAILURE;
            }
            if (table) { coll.kmers_k = k; coll.kmers_path = argv[i + 2]; }
            else { coll.sharing_k = k; coll.sharing_path = argv[i + 2]; }
            i += 2;
        }
        else if (std::strcmp(argv[i], "--min-docs") == 0 || std::strcmp(argv[i], "--max-docs") == 0) {
            const bool lo = std::strcmp(argv[i], "--min-docs") == 0;
            size_t v = 0;
            if (i + 1 >= argc || !parse_count(argv[i + 1], v) || v < 1) { std::cerr << argv[i] << ": a number of documents of at least 1, please\n"; return EXIT_FAILURE; }
            (lo ? coll.min_docs : coll.max_docs) = v;
            (lo ? min_docs_given : max_docs_given) = true;
            ++i;
        }
        else if (std::strcmp(argv[i], "--kmers") == 0 || std::strcmp(argv[i], "--kmer-spectrum") == 0) {
            const bool table = std::strcmp(argv[i], "--kmers") == 0;
            const char* opt = argv[i];
            size_t k = 0;
            if ((table ? kmers : spectrum)) { std::cerr << opt << ": given twice\n"; return EXIT_FAILURE; }
            if (i + 2 >= argc || !parse_count(argv[i + 1], k) || k < 1 || std::strncmp(argv[i + 2], "--", 2) == 0) {
                std::cerr << opt << ": usage: " << opt << " K PATH (K >= 1)\n";
                return EXIT_FAILURE;
            }
            if (table) { kmers = true; km.k = k; km.path = argv[i + 2]; }
            else { spectrum = true; km.spectrum_k = k; km.spectrum_path = argv[i + 2]; }
            i += 2;
        }
        else if (std::strcmp(argv[i], "--lz77") == 0) {
            if (lz) { std::cerr << "--lz77: given twice\n"; return EXIT_FAILURE; }
            if (i + 1 >= argc || std::strncmp(argv[i + 1], "--", 2) == 0) { std::cerr << "--lz77: usage: --lz77 PATH\n"; return EXIT_FAILURE; }
            lz = true;
            lz_path = argv[++i];
        }
        else if (std::strcmp(argv[i], "--lce-index") == 0) {
            if (lce) { std::cerr << "--lce-index: given twice\n"; return EXIT_FAILURE; }
            if (i + 1 >= argc || std::strncmp(argv[i + 1], "--", 2) == 0) { std::cerr << "--lce-index: usage: --lce-index PATH\n"; return EXIT_FAILURE; }
            lce = true;
            lce_path = argv[++i];
        }
        else if (std::strcmp(argv[i], "--cross-mums") == 0 || std::strcmp(argv[i], "--cross-mems") == 0) {
            const bool mems = std::strcmp(argv[i], "--cross-mems") == 0;
            const char* opt = argv[i];
            size_t split = 0;
            if (!(mems ? cross.mems_path : cross.mums_path).empty()) { std::cerr << opt << ": given twice\n"; return EXIT_FAILURE; }
            if (i + 2 >= argc || !parse_count(argv[i + 1], split) || std::strncmp(argv[i + 2], "--", 2) == 0 || !argv[i + 2][0]) {
                std::cerr << opt << ": usage: " << opt << " SPLIT PATH\n";
                return EXIT_FAILURE;
            }
            (mems ? cross.mems_split : cross.mums_split) = split;
            (mems ? cross.mems_path : cross.mums_path) = argv[i + 2];
            i += 2;
        }
        else if (std::strcmp(argv[i], "--max-occ") == 0) {
            if (i + 1 >= argc || !parse_count(argv[i + 1], cross.max_occ) || cross.max_occ < 2 || cross.max_occ > 64) {
                std::cerr << "--max-occ: a number in 2 .. 64, please\n";
                return EXIT_FAILURE;
            }
            max_occ_given = true;
            ++i;
        }
        else if (std::strcmp(argv[i], "--mismatches") == 0) { std::cerr << "--mismatches: only with --lce\n"; return EXIT_FAILURE; }
        else if (std::strcmp(argv[i], "--min-count") == 0 || std::strcmp(argv[i], "--max-count") == 0) {
            const bool lo = std::strcmp(argv[i], "--min-count") == 0;
            size_t v = 0;
            if (i + 1 >= argc || !parse_count(argv[i + 1], v) || v < 1) { std::cerr << argv[i] << ": a count of at least 1, please\n"; return EXIT_FAILURE; }
            (lo ? km.min_count : km.max_count) = v;
            (lo ? min_count_given : max_count_given) = true;
            ++i;
        }
        else if (std::strcmp(argv[i], "--raw") == 0) raw = true;
        else if (std::strcmp(argv[i], "--bwt") == 0) {
            bwt = true;
            if (i + 1 < argc && std::strncmp(argv[i + 1], "--", 2) != 0) bwt_path = argv[++i];
        }
        else if (std::strcmp(argv[i], "--fm-index") == 0) {
            fm = true;
            if (i + 1 < argc && std::strncmp(argv[i + 1], "--", 2) != 0) fm_path = argv[++i];
        }
        else if (std::strcmp(argv[i], "--fm-sample") == 0) {
            fm_sample_given = true;
            if (i + 1 >= argc || !parse_count(argv[++i], fm_sample) || fm_sample < 1 || fm_sample > 1024 || (fm_sample & (fm_sample - 1))) {
                std::cerr << "--fm-sample: a power of two in 1 .. 1024, please\n";
                return EXIT_FAILURE;
            }
        }
        else if (std::strcmp(argv[i], "--fm-text-sample") == 0) {
            fm_text_given = true;
            if (i + 1 >= argc || !parse_count(argv[++i], fm_text_sample) || fm_text_sample < 1 || fm_text_sample > 1024 ||
                (fm_text_sample & (fm_text_sample - 1))) {
                std::cerr << "--fm-text-sample: a power of two in the --fm-sample distance .. 1024, please\n";
                return EXIT_FAILURE;
            }
        }
        else if (std::strcmp(argv[i], "--locate") == 0) { std::cerr << "--locate: only with --fm-search\n"; return EXIT_FAILURE; }
        else if (std::strcmp(argv[i], "--min-len") == 0) {      // (with --cross-mums / --cross-mems; checked behind the loop)
            min_len_given = true;
            if (i + 1 < argc && parse_count(argv[i + 1], cross.min_len)) ++i;
            else cross.min_len = 0;
        }
        else if (std::strcmp(argv[i], "--gpus") == 0 && i + 1 < argc) {
            if (!parse_count(argv[++i], gpus) || gpus < 1 || gpus > 64) { std::cerr << "--gpus: a device count, please\n"; return EXIT_FAILURE; }
        } else pos.push_back(argv[i]);
    }
    if (min_len_given && !cross.any()) { std::cerr << "--min-len: only with --fm-mems\n"; return EXIT_FAILURE; }
    if (pos.size() < 2) {
        std::cerr << "Usage: caps_sa <input_path> <output_path> <(optional)-subproblem-count> "
                     "<(optional)-bounded-context> <(optional)--pretty-print> <(optional)--gpus N> <(optional)--bwt PATH> "
                     "<(optional)--fm-index PATH [--fm-sample S] [--fm-text-sample T]> <(optional)--raw> "
                     "<(optional)--kmers K PATH [--min-count A] [--max-count B]> <(optional)--kmer-spectrum K PATH> <(optional)--lz77 PATH> "
                     "<(optional)--lce-index PATH> <(optional)--cross-mums SPLIT PATH [--min-len L]> <(optional)--cross-mems SPLIT PATH [--min-len L] [--max-occ C]> "
                     "<(optional)--docs FILE --kmer-sharing K PATH --coll-kmers K PATH [--min-docs A] [--max-docs B]>\n"
                     "       caps_sa --lce INDEX PAIRS [--mismatches K]\n"
                     "       caps_sa --inverse-bwt IN.bwt OUT\n"
                     "       caps_sa --fm-search INDEX PATTERNS [--locate K]\n"
                     "       caps_sa --fm-mems INDEX PATTERNS [--min-len L]\n"
                     "       caps_sa --fm-from-bwt IN.bwt OUT.fm [--fm-sample S] [--fm-text-sample T]\n"
                     "       caps_sa --fm-extract INDEX RANGES\n";
        return EXIT_FAILURE;
    }
    size_t p = 0, ctx = 0;
    if (pos.size() >= 3 && !parse_count(pos[2], p)) { std::cerr << "subproblem-count: not a number: " << pos[2] << "\n"; return EXIT_FAILURE; }
    if (pos.size() >= 4 && !parse_count(pos[3], ctx)) { std::cerr << "bounded-context: not a number: " << pos[3] << "\n"; return EXIT_FAILURE; }
    // --bwt: refused before any file is opened (the input's size comes from stat())
    if (bwt) {
        if (bwt_path.empty()) { std::cerr << "--bwt: missing output path (--bwt PATH)\n"; return EXIT_FAILURE; }
        if (gpus > 1) { std::cerr << "--bwt: the BWT is built on one GPU; --gpus " << gpus << " has no BWT output\n"; return EXIT_FAILURE; }
        struct stat sb;                                       // (an input that cannot be stat'ed is reported by read_input below)
        if (ctx != 0 && stat(pos[0].c_str(), &sb) == 0 && ctx < static_cast<size_t>(sb.st_size)) {
            std::cerr << "--bwt: a bounded-context order (bounded-context " << ctx << ") is not a suffix array and has no BWT\n";
            return EXIT_FAILURE;
        }
    }
    // --kmers / --kmer-spectrum: the same manners
#ifdef CAPS_CLI_NO_KMERS
    if (kmers || spectrum) { std::cerr << (kmers ? "--kmers" : "--kmer-spectrum") << ": not built into this driver\n"; return EXIT_FAILURE; }
#endif
    if (min_count_given && !kmers) { std::cerr << "--min-count: only with --kmers K PATH\n"; return EXIT_FAILURE; }
    if (max_count_given && !kmers) { std::cerr << "--max-count: only with --kmers K PATH\n"; return EXIT_FAILURE; }
    if (kmers && raw) { std::cerr << "--kmers: the table is lines of text, and --raw keeps arbitrary bytes that do not make lines (--kmer-spectrum works with --raw)\n"; return EXIT_FAILURE; }
    if (kmers && max_count_given && km.min_count > km.max_count) { std::cerr << "--kmers: --min-count " << km.min_count << " is above --max-count " << km.max_count << "\n"; return EXIT_FAILURE; }
    if (kmers || spectrum) {
        const char* opt = kmers ? "--kmers" : "--kmer-spectrum";
        struct stat sb;
        if (ctx != 0 && stat(pos[0].c_str(), &sb) == 0 && ctx < static_cast<size_t>(sb.st_size)) {
            std::cerr << opt << ": a bounded-context order (bounded-context " << ctx << ") is not a suffix array and has no k-mer table\n";
            return EXIT_FAILURE;
        }
    }
    // --lz77: the same manners
#ifdef CAPS_CLI_NO_LZ
    if (lz) { std::cerr << "--lz77: not built into this driver\n"; return EXIT_FAILURE; }
#endif
    if (lz) {
        struct stat sb;
        if (ctx != 0 && stat(pos[0].c_str(), &sb) == 0 && ctx < static_cast<size_t>(sb.st_size)) {
            std::cerr << "--lz77: a bounded-context order (bounded-context " << ctx << ") is not a suffix array and has no LZ77 factorization\n";
            return EXIT_FAILURE;
        }
    }
    // --lce-index: the same manners
#ifdef CAPS_CLI_NO_LCE
    if (lce) { std::cerr << "--lce-index: not built into this driver\n"; return EXIT_FAILURE; }
#endif
    if (lce) {
        struct stat sb;
        if (ctx != 0 && stat(pos[0].c_str(), &sb) == 0 && ctx < static_cast<size_t>(sb.st_size)) {
            std::cerr << "--lce-index: a bounded-context order (bounded-context " << ctx << ") is not a suffix array and has no LCE index\n";
            return EXIT_FAILURE;
        }
    }
    // --cross-mums / --cross-mems: the same manners
#ifdef CAPS_CLI_NO_CROSS
    if (cross.any()) { std::cerr << (cross.mums_path.empty() ? "--cross-mems" : "--cross-mums") << ": not built into this driver\n"; return EXIT_FAILURE; }
#endif
    if (max_occ_given && cross.mems_path.empty()) { std::cerr << "--max-occ: only with --cross-mems SPLIT PATH\n"; return EXIT_FAILURE; }
    if (cross.any()) {
        const char* opt = cross.mums_path.empty() ? "--cross-mems" : "--cross-mums";
        if (min_len_given && cross.min_len < 1) { std::cerr << "--min-len: a length of at least 1, please\n"; return EXIT_FAILURE; }
        if (gpus > 1) { std::cerr << opt << ": the matches need the BWT, which is built on one GPU; --gpus " << gpus << " has none\n"; return EXIT_FAILURE; }
        struct stat sb;
        if (stat(pos[0].c_str(), &sb) == 0) {
            const size_t n = static_cast<size_t>(sb.st_size);
            if (ctx != 0 && ctx < n) {
                std::cerr << opt << ": a bounded-context order (bounded-context " << ctx << ") is not a suffix array and has no matches between two texts\n";
                return EXIT_FAILURE;
            }
            if ((!cross.mums_path.empty() && cross.mums_split > n) || (!cross.mems_path.empty() && cross.mems_split > n)) {
                std::cerr << opt << ": SPLIT is beyond the text (n = " << n << ")\n";
                return EXIT_FAILURE;
            }
        }
    }
    // --docs / --kmer-sharing / --coll-kmers: the same manners
#ifdef CAPS_CLI_NO_COLL
    if (coll.any() || docs_given) { std::cerr << (coll.kmers_k ? "--coll-kmers" : coll.sharing_k ? "--kmer-sharing" : "--docs") << ": not built into this driver\n"; return EXIT_FAILURE; }
#endif
    if (min_docs_given && !coll.kmers_k) { std::cerr << "--min-docs: only with --coll-kmers K PATH\n"; return EXIT_FAILURE; }
    if (max_docs_given && !coll.kmers_k) { std::cerr << "--max-docs: only with --coll-kmers K PATH\n"; return EXIT_FAILURE; }
    if (docs_given && !coll.any()) { std::cerr << "--docs: only with --kmer-sharing K PATH or --coll-kmers K PATH\n"; return EXIT_FAILURE; }
    if (coll.any()) {
        const char* opt = coll.kmers_k ? "--coll-kmers" : "--kmer-sharing";
        if (!docs_given) { std::cerr << opt << ": needs --docs FILE (one `start length` per line)\n"; return EXIT_FAILURE; }
        if (coll.kmers_k && raw) { std::cerr << "--coll-kmers: the table is lines of text, and --raw keeps arbitrary bytes that do not make lines (--kmer-sharing works with --raw)\n"; return EXIT_FAILURE; }
        if (max_docs_given && coll.min_docs > coll.max_docs) { std::cerr << "--coll-kmers: --min-docs " << coll.min_docs << " is above --max-docs " << coll.max_docs << "\n"; return EXIT_FAILURE; }
        struct stat sb;
        if (stat(pos[0].c_str(), &sb) != 0) { std::cerr << pos[0] << " : cannot open\n"; return EXIT_FAILURE; }
        const size_t n = static_cast<size_t>(sb.st_size);
        if (ctx != 0 && ctx < n) {
            std::cerr << opt << ": a bounded-context order (bounded-context " << ctx << ") is not a suffix array and has no k-mer table\n";
            return EXIT_FAILURE;
        }
        std::string why;
        if (!read_docs(docs_path, n, coll.docs, why)) { std::cerr << "--docs: " << why << "\n"; return EXIT_FAILURE; }
    }
    // --fm-index: the same manners
    if (fm_sample_given && !fm) { std::cerr << "--fm-sample: only with --fm-index PATH\n"; return EXIT_FAILURE; }
    if (fm_text_given && !fm) { std::cerr << "--fm-text-sample: only with --fm-index PATH or --fm-from-bwt\n"; return EXIT_FAILURE; }
    if (fm_text_given && fm_text_sample < fm_sample) {
        std::cerr << "--fm-text-sample: a power of two in the --fm-sample distance .. 1024, please (--fm-sample is " << fm_sample << ")\n";
        return EXIT_FAILURE;
    }
    if (raw && fm_text_given) {
        std::cerr << "--fm-text-sample: --raw --fm-index writes a wide FM-index (\"CAPSFMW1\"): text samples are not built for the wide format\n";
        return EXIT_FAILURE;
    }
    if (fm) {
        if (fm_path.empty()) { std::cerr << "--fm-index: missing output path (--fm-index PATH)\n"; return EXIT_FAILURE; }
        if (gpus > 1) { std::cerr << "--fm-index: the index is built on one GPU; --gpus " << gpus << " has no BWT to build it from\n"; return EXIT_FAILURE; }
        struct stat sb;
        if (ctx != 0 && stat(pos[0].c_str(), &sb) == 0 && ctx < static_cast<size_t>(sb.st_size)) {
            std::cerr << "--fm-index: a bounded-context order (bounded-context " << ctx << ") is not a suffix array and has no FM-index\n";
            return EXIT_FAILURE;
        }
    }

    std::string text;
    if (!read_input(pos[0], text)) return EXIT_FAILURE;
    // the byte remap of main.cpp:61-70, on all host threads like the reference's parallel_for (--raw: the text as given)
    if (!raw) {
        static const char lookup[4] = {'A', 'C', 'T', 'G'};
        const size_t n = text.size();
        const size_t nt = std::max<size_t>(1, std::min<size_t>(std::thread::hardware_concurrency(), n / (1u << 20) + 1));
        std::vector<std::thread> th;
        char* d = &text[0];
        for (size_t t = 0; t < nt; ++t)
            th.emplace_back([=]() {
                for (size_t j = n * t / nt, e = n * (t + 1) / nt; j < e; ++j)
                    d[j] = lookup[(std::toupper(static_cast<unsigned char>(d[j])) & 0x6) >> 1];
            });
        for (auto& t : th) t.join();
    }
    std::vector<int> devices;
    for (size_t i = 0; i < gpus; ++i) devices.push_back(static_cast<int>(i));

    std::cerr << "Text length: " << text.size() << ".\n";
    try {
        if (text.size() <= std::numeric_limits<uint32_t>::max()) return run<uint32_t>(text, pos[1], p, ctx, pretty, devices, bwt_path, fm_path, (uint32_t)fm_sample, (uint32_t)fm_text_sample, raw, km, lz_path, lce_path, cross, coll);
        return run<uint64_t>(text, pos[1], p, ctx, pretty, devices, bwt_path, fm_path, (uint32_t)fm_sample, (uint32_t)fm_text_sample, raw, km, lz_path, lce_path, cross, coll);
    } catch (const std::exception& e) {
        std::cerr << e.what() << "\n";
        return EXIT_FAILURE;
    }
}
