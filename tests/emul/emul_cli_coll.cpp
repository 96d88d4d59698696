// tests/emul/emul_cli_coll.cpp -- emul_cli_cross.cpp plus the collection k-mer entry points (test infrastructure only).
//
// The host entry points of include/caps_sa_hip.h "k-mers across a collection" renamed to their emulation twins, then the driver of
// emul_cli_cross.cpp as it is.  tests/test_cli_coll.py builds it:
//     g++ -O2 -std=c++17 -o caps_sa_emul_coll emul_cli_coll.cpp -L. -lcaps_sa_emul -Wl,-rpath,<this directory>
#define caps_sa_hip_coll_kmers_u32 caps_sa_emul_coll_kmers_u32
#define caps_sa_hip_coll_kmers_u64 caps_sa_emul_coll_kmers_u64
#define caps_sa_hip_coll_sharing_u32 caps_sa_emul_coll_sharing_u32
#define caps_sa_hip_coll_sharing_u64 caps_sa_emul_coll_sharing_u64

#include "emul_cli_cross.cpp"
