// tests/emul/emul_cli_lz.cpp -- emul_cli_kmers.cpp plus the LZ77 entry points (test infrastructure only).
//
// The host entry points of include/caps_sa_hip.h "LPF and LZ77 from SA and LCP" renamed to their emulation twins, then the driver of
// emul_cli_kmers.cpp as it is.  tests/test_cli_lz.py builds it:
//     g++ -O2 -std=c++17 -o caps_sa_emul_lz emul_cli_lz.cpp -L. -lcaps_sa_emul -Wl,-rpath,<this directory>
#define caps_sa_hip_lpf_u32 caps_sa_emul_lpf_u32
#define caps_sa_hip_lpf_u64 caps_sa_emul_lpf_u64
#define caps_sa_hip_lz77_u32 caps_sa_emul_lz77_u32
#define caps_sa_hip_lz77_u64 caps_sa_emul_lz77_u64

#include "emul_cli_kmers.cpp"
