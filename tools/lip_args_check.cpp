// Stand-alone host check of the argument validation of mf_melspec_windows and mf_wav2lip_forward_u8_rows: every call below must be refused with MF_ERR_INVALID
// before anything touches a device, so the program runs on a box without a GPU -- built with the host side under AddressSanitizer + UBSan:
//
//   for f in mere-fusion_amd/csrc/*.hip mere-fusion_amd/csrc/mf_api.cpp tools/lip_args_check.cpp; do
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -Iinclude -mllvm -pragma-unroll-threshold=262144 -Xarch_host -fsanitize=address,undefined -c $f -o OBJ/$(basename $f).o; done
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined OBJ/*.o -o lip_args_check && ./lip_args_check
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
#include "merefusion.h"

static int failures = 0;
static void expect(int rc, const char* needle, const char* what) {
    const char* err = mf_last_error();
    const bool ok = rc == -1 && err && std::strstr(err, needle);
    std::printf("%-58s rc=%d  %s\n", what, rc, err ? err : "(no message)");
    if (!ok) { ++failures; std::printf("    ^^^ expected MF_ERR_INVALID with '%s'\n", needle); }
}

int main() {
    const int n = 24 * 320, T = 1 + n / 200;
    std::vector<float> host(16);                       // never dereferenced: every call is refused first
    float* p = host.data();
    const uint8_t* pool = reinterpret_cast<const uint8_t*>(host.data());
    int ok[2] = {16, 19};
    expect(mf_melspec_windows(p, 0, 1, ok, 2, p, 0, nullptr), "empty signal", "melspec_windows n = 0");
    expect(mf_melspec_windows(p, -7, 1, ok, 2, p, 0, nullptr), "empty signal", "melspec_windows n < 0");
    expect(mf_melspec_windows(p, n, 0, ok, 2, p, 0, nullptr), "n_windows", "melspec_windows n_windows = 0");
    expect(mf_melspec_windows(p, n, -1, ok, 2, p, 0, nullptr), "n_windows", "melspec_windows n_windows < 0");
    expect(mf_melspec_windows(nullptr, n, 1, ok, 2, p, 0, nullptr), "null", "melspec_windows wav = NULL");
    expect(mf_melspec_windows(p, n, 1, nullptr, 2, p, 0, nullptr), "null", "melspec_windows starts = NULL");
    expect(mf_melspec_windows(p, n, 1, ok, 2, nullptr, 0, nullptr), "null", "melspec_windows chunks = NULL");
    expect(mf_melspec_windows(p, n, 1, ok, 0, p, 0, nullptr), "chunk starts", "melspec_windows n_starts = 0");
    expect(mf_melspec_windows(p, n, 1, ok, 257, p, 0, nullptr), "chunk starts", "melspec_windows n_starts = 257 (only 2 readable)");
    expect(mf_melspec_windows(p, n, 1, ok, 2, p, 2, nullptr), "pad_mode", "melspec_windows pad_mode = 2");
    int z[1] = {0};
    expect(mf_melspec_windows(p, 400, 1, z, 1, p, 1, nullptr), "reflect", "melspec_windows reflect, n = 400");
    const int bad_starts[4] = {-1, T - 15, T, 1 << 30};
    for (int b : bad_starts) {
        int st[2] = {16, b};
        expect(mf_melspec_windows(p, n, 1, st, 2, p, 0, nullptr), "outside", "melspec_windows start outside [0, T - 16]");
    }
    mf_wav2lip* h = reinterpret_cast<mf_wav2lip*>(host.data());   // never dereferenced either
    int rows[2] = {0, 11};
    expect(mf_wav2lip_forward_u8_rows(nullptr, p, pool, 12, rows, p, 2, nullptr), "null", "forward_u8_rows handle = NULL");
    expect(mf_wav2lip_forward_u8_rows(h, nullptr, pool, 12, rows, p, 2, nullptr), "null", "forward_u8_rows mel = NULL");
    expect(mf_wav2lip_forward_u8_rows(h, p, nullptr, 12, rows, p, 2, nullptr), "null", "forward_u8_rows pool = NULL");
    expect(mf_wav2lip_forward_u8_rows(h, p, pool, 12, nullptr, p, 2, nullptr), "null", "forward_u8_rows rows = NULL");
    expect(mf_wav2lip_forward_u8_rows(h, p, pool, 12, rows, nullptr, 2, nullptr), "null", "forward_u8_rows frames = NULL");
    expect(mf_wav2lip_forward_u8_rows(h, p, pool, 12, rows, p, 0, nullptr), "batch", "forward_u8_rows batch = 0");
    expect(mf_wav2lip_forward_u8_rows(h, p, pool, 0, rows, p, 2, nullptr), "pool", "forward_u8_rows n_pool_rows = 0");
    const int bad_rows[3] = {-1, 12, 1 << 30};
    for (int b : bad_rows) {
        int r[2] = {3, b};
        expect(mf_wav2lip_forward_u8_rows(h, p, pool, 12, r, p, 2, nullptr), "out of range", "forward_u8_rows row outside the pool");
    }
    std::printf(failures ? "%d FAILED\n" : "all refused as expected (%d failures)\n", failures);
    return failures ? 1 : 0;
}
