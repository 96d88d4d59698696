// tests/emul/emul_cli.cpp -- the command-line driver over the host emulation (test infrastructure only).
//
// The CLI's own source (caps-sa_amd/csrc/caps_sa_cli.cpp) and the C++ classes it uses, compiled with every entry point of the C ABI
// they call renamed to its emulation twin (emul_lib.cpp exports the same ABI as caps_sa_emul_*), and linked against
// libcaps_sa_emul.so.  What the CLI does end to end -- remap, build, the files it writes, the lines it prints -- runs without a GPU.
// tests/test_cli_fm_wide.py builds it:
//     g++ -O2 -std=c++17 -o caps_sa_emul emul_cli.cpp -L. -lcaps_sa_emul -Wl,-rpath,<this directory>
#define caps_sa_hip_last_error caps_sa_emul_last_error
#define caps_sa_hip_host_alloc caps_sa_emul_host_alloc
#define caps_sa_hip_host_free caps_sa_emul_host_free
#define caps_sa_hip_build_multi_u32 caps_sa_emul_build_multi_u32
#define caps_sa_hip_build_multi_u64 caps_sa_emul_build_multi_u64
#define caps_sa_hip_build_bwt_u32 caps_sa_emul_build_bwt_u32
#define caps_sa_hip_build_bwt_u64 caps_sa_emul_build_bwt_u64
#define caps_sa_hip_inverse_bwt_u32 caps_sa_emul_inverse_bwt_u32
#define caps_sa_hip_inverse_bwt_u64 caps_sa_emul_inverse_bwt_u64
#define caps_sa_hip_fm_index_bytes caps_sa_emul_fm_index_bytes
#define caps_sa_hip_fm_index_bytes_ex caps_sa_emul_fm_index_bytes_ex
#define caps_sa_hip_fm_build_u32 caps_sa_emul_fm_build_u32
#define caps_sa_hip_fm_build_u64 caps_sa_emul_fm_build_u64
#define caps_sa_hip_fm_build_from_bwt_u32 caps_sa_emul_fm_build_from_bwt_u32
#define caps_sa_hip_fm_build_from_bwt_u64 caps_sa_emul_fm_build_from_bwt_u64
#define caps_sa_hip_fm_wide_index_bytes caps_sa_emul_fm_wide_index_bytes
#define caps_sa_hip_fm_build_wide_u32 caps_sa_emul_fm_build_wide_u32
#define caps_sa_hip_fm_build_wide_u64 caps_sa_emul_fm_build_wide_u64
#define caps_sa_hip_fm_count caps_sa_emul_fm_count
#define caps_sa_hip_fm_locate caps_sa_emul_fm_locate
#define caps_sa_hip_fm_match caps_sa_emul_fm_match
#define caps_sa_hip_fm_mems caps_sa_emul_fm_mems
#define caps_sa_hip_fm_add_text_samples caps_sa_emul_fm_add_text_samples
#define caps_sa_hip_fm_extract caps_sa_emul_fm_extract

#include "../../caps-sa_amd/csrc/caps_sa_cli.cpp"
