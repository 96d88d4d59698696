// tests/emul/emul_cli_lce.cpp -- emul_cli_lz.cpp plus the ISA and LCE entry points (test infrastructure only).
//
// The host entry points of include/caps_sa_hip.h "ISA and longest common extensions" renamed to their emulation twins, then the driver
// of emul_cli_lz.cpp as it is.  tests/test_cli_lce.py builds it:
//     g++ -O2 -std=c++17 -o caps_sa_emul_lce emul_cli_lce.cpp -L. -lcaps_sa_emul -Wl,-rpath,<this directory>
#define caps_sa_hip_isa_u32 caps_sa_emul_isa_u32
#define caps_sa_hip_isa_u64 caps_sa_emul_isa_u64
#define caps_sa_hip_lce_index_bytes caps_sa_emul_lce_index_bytes
#define caps_sa_hip_lce_build_u32 caps_sa_emul_lce_build_u32
#define caps_sa_hip_lce_build_u64 caps_sa_emul_lce_build_u64
#define caps_sa_hip_lce_range_min caps_sa_emul_lce_range_min
#define caps_sa_hip_lce caps_sa_emul_lce

#include "emul_cli_lz.cpp"
