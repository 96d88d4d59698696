// tests/emul/emul_cli_kmers.cpp -- emul_cli.cpp plus the k-mer entry points (test infrastructure only).
//
// The host entry points of include/caps_sa_hip.h "k-mers from SA and LCP" renamed to their emulation twins, then the driver of
// emul_cli.cpp as it is.  tests/test_cli_kmers.py builds it:
//     g++ -O2 -std=c++17 -o caps_sa_emul_kmers emul_cli_kmers.cpp -L. -lcaps_sa_emul -Wl,-rpath,<this directory>
#define caps_sa_hip_kmers_u32 caps_sa_emul_kmers_u32
#define caps_sa_hip_kmers_u64 caps_sa_emul_kmers_u64
#define caps_sa_hip_kmer_spectrum_u32 caps_sa_emul_kmer_spectrum_u32
#define caps_sa_hip_kmer_spectrum_u64 caps_sa_emul_kmer_spectrum_u64
#define caps_sa_hip_kmer_census_u32 caps_sa_emul_kmer_census_u32
#define caps_sa_hip_kmer_census_u64 caps_sa_emul_kmer_census_u64

#include "emul_cli.cpp"
