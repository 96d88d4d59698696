// tests/emul/emul_cli_cross.cpp -- emul_cli_lce.cpp plus the MUM / MEM entry points (test infrastructure only).
//
// The host entry points of include/caps_sa_hip.h "MUMs and MEMs between two texts" renamed to their emulation twins, then the driver
// of emul_cli_lce.cpp as it is.  tests/test_cli_cross.py builds it:
//     g++ -O2 -std=c++17 -o caps_sa_emul_cross emul_cli_cross.cpp -L. -lcaps_sa_emul -Wl,-rpath,<this directory>
#define caps_sa_hip_cross_mums_u32 caps_sa_emul_cross_mums_u32
#define caps_sa_hip_cross_mums_u64 caps_sa_emul_cross_mums_u64
#define caps_sa_hip_cross_mems_u32 caps_sa_emul_cross_mems_u32
#define caps_sa_hip_cross_mems_u64 caps_sa_emul_cross_mems_u64

#include "emul_cli_lce.cpp"
