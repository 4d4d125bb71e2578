// Stand-alone host check of the argument validation of mf_nerf_feat_scatter, mf_nerf_feat_windows and mf_nerf_feat_rows_load: every call below must be refused with MF_ERR_INVALID
// before anything touches a device, so the program runs on a box without a GPU -- built with the host side under AddressSanitizer + UBSan:
//
//   for f in mere-fusion_amd/csrc/mf_nerf_featpool.hip mere-fusion_amd/csrc/mf_api.cpp tools/nerf_featpool_args_check.cpp; do
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -Iinclude -Xarch_host -fsanitize=address,undefined -c $f -o OBJ/$(basename $f).o; done
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined OBJ/*.o -o nerf_featpool_args_check && ./nerf_featpool_args_check
//
// The host arrays are exactly as long as the arguments say, so a check that read past them (or before refusing a count) would be reported.
#include <cstdio>
#include <cstring>
#include <vector>
#include "merefusion.h"

static int failures = 0;
static void expect(int rc, const char* needle, const char* what) {
    const char* err = mf_last_error();
    const bool ok = rc == -1 && err && std::strstr(err, needle);
    std::printf("%-62s rc=%d  %s\n", what, rc, err ? err : "(no message)");
    if (!ok) { ++failures; std::printf("    ^^^ expected MF_ERR_INVALID with '%s'\n", needle); }
}

int main() {
    std::vector<float> host(16);                       // never dereferenced: every call is refused first
    float* p = host.data();
    const int N = 3, R = 32, T = 27;
    std::vector<int> rows{0, 2}, starts{16, 24};
    auto scatter = [&](const float* feats, int S, int t, int dim, int left, int right, float* rings, int n, int r, const int* rw, const int* st) {
        return mf_nerf_feat_scatter(feats, S, t, dim, left, right, rings, n, r, rw, st, nullptr);
    };
    expect(scatter(nullptr, 2, T, 44, 10, 18, p, N, R, rows.data(), starts.data()), "null", "scatter feats = NULL");
    expect(scatter(p, 2, T, 44, 10, 18, nullptr, N, R, rows.data(), starts.data()), "null", "scatter rings = NULL");
    expect(scatter(p, 2, T, 44, 10, 18, p, N, R, nullptr, starts.data()), "null", "scatter rows = NULL");
    expect(scatter(p, 2, T, 44, 10, 18, p, N, R, rows.data(), nullptr), "null", "scatter starts = NULL");
    for (int dim : {0, -1, 1025, 1 << 30}) expect(scatter(p, 2, T, dim, 10, 18, p, N, R, rows.data(), starts.data()), "dim", "scatter dim outside 1..1024");
    for (int r : {15, 0, -32, 1 << 30}) expect(scatter(p, 2, T, 44, 10, 18, p, N, r, rows.data(), starts.data()), "ring", "scatter R outside 16..65536");
    for (int n : {0, -1, 1 << 30}) expect(scatter(p, 2, T, 44, 10, 18, p, n, R, rows.data(), starts.data()), "pool", "scatter N outside 1..65536");
    for (int S : {0, -2, 4, 1 << 30}) expect(scatter(p, S, T, 44, 10, 18, p, N, R, rows.data(), starts.data()), "picked", "scatter n_sessions outside 1..N (2 readable)");
    expect(scatter(p, 2, 0, 44, 10, 18, p, N, R, rows.data(), starts.data()), "net frames", "scatter T = 0");
    expect(scatter(p, 2, T, 44, -1, 18, p, N, R, rows.data(), starts.data()), "net frames", "scatter left < 0");
    expect(scatter(p, 2, T, 44, 18, 18, p, N, R, rows.data(), starts.data()), "net frames", "scatter left = right");
    expect(scatter(p, 2, T, 44, 10, 28, p, N, R, rows.data(), starts.data()), "net frames", "scatter right > T");
    for (int b : {-1, 3, 1 << 30}) {
        std::vector<int> r{0, b};
        expect(scatter(p, 2, T, 44, 10, 18, p, N, R, r.data(), starts.data()), "out of range", "scatter row outside the pool");
    }
    std::vector<int> twice{2, 2};
    expect(scatter(p, 2, T, 44, 10, 18, p, N, R, twice.data(), starts.data()), "twice", "scatter a row twice");
    for (int b : {-1, 25, 2147483647}) {
        std::vector<int> st{16, b};
        expect(scatter(p, 2, T, 44, 10, 18, p, N, R, rows.data(), st.data()), "leave the ring", "scatter 8 rows leave the ring");
    }

    const std::vector<int> fronts{-1, -1, -1, -1, 24, 26, 28, 30, 2, 4, 6, 8, 10, 12, 14, 16};
    std::vector<int> heads{4, 7}, n_new{4, 1};
    auto windows = [&](const float* rings, float* hist, int n, int r, int dim, int S, const int* rw, const int* fr, const int* hd, const int* nn, int att, float* out) {
        return mf_nerf_feat_windows(rings, hist, n, r, dim, S, rw, fr, hd, nn, att, out, nullptr);
    };
    expect(windows(nullptr, p, N, R, 1024, 2, rows.data(), fronts.data(), heads.data(), n_new.data(), 1, p), "null", "windows rings = NULL");
    expect(windows(p, p, N, R, 1024, 2, nullptr, fronts.data(), heads.data(), n_new.data(), 1, p), "null", "windows rows = NULL");
    expect(windows(p, p, N, R, 1024, 2, rows.data(), nullptr, heads.data(), n_new.data(), 1, p), "null", "windows fronts = NULL");
    expect(windows(p, p, N, R, 1024, 2, rows.data(), fronts.data(), heads.data(), nullptr, 1, p), "null", "windows n_new = NULL");
    expect(windows(p, p, N, R, 1024, 2, rows.data(), fronts.data(), heads.data(), n_new.data(), 1, nullptr), "null", "windows out = NULL");
    expect(windows(p, nullptr, N, R, 1024, 2, rows.data(), fronts.data(), heads.data(), n_new.data(), 1, p), "null history", "windows att without hist");
    expect(windows(p, p, N, R, 1024, 2, rows.data(), fronts.data(), nullptr, n_new.data(), 1, p), "null history", "windows att without heads");
    for (int dim : {0, -1, 1025}) expect(windows(p, p, N, R, dim, 2, rows.data(), fronts.data(), heads.data(), n_new.data(), 1, p), "dim", "windows dim outside 1..1024");
    for (int r : {15, -32, 1 << 30}) expect(windows(p, p, N, r, 1024, 2, rows.data(), fronts.data(), heads.data(), n_new.data(), 1, p), "ring", "windows R outside 16..65536");
    for (int n : {0, 1 << 30}) expect(windows(p, p, n, R, 1024, 2, rows.data(), fronts.data(), heads.data(), n_new.data(), 1, p), "pool", "windows N outside 1..65536");
    for (int S : {0, -2, 4}) expect(windows(p, p, N, R, 1024, S, rows.data(), fronts.data(), heads.data(), n_new.data(), 1, p), "picked", "windows n_sessions outside 1..N");
    for (int b : {-1, 3, 1 << 30}) {
        std::vector<int> r{0, b};
        expect(windows(p, p, N, R, 1024, 2, r.data(), fronts.data(), heads.data(), n_new.data(), 1, p), "out of range", "windows row outside the pool");
    }
    expect(windows(p, p, N, R, 1024, 2, twice.data(), fronts.data(), heads.data(), n_new.data(), 1, p), "twice", "windows a row twice");
    const int bad_fronts[5][2] = {{7, 32}, {0, -2}, {4, -1}, {15, -1}, {8, 1 << 30}};   // (window, value): new windows (4..7, 15) must start inside the ring
    for (const auto& b : bad_fronts) {
        std::vector<int> f(fronts);
        f[b[0]] = b[1];
        expect(windows(p, p, N, R, 1024, 2, rows.data(), f.data(), heads.data(), n_new.data(), 1, p), "front", "windows front outside the ring");
    }
    for (int b : {-1, 8}) {
        std::vector<int> h{b, 0};
        expect(windows(p, p, N, R, 1024, 2, rows.data(), fronts.data(), h.data(), n_new.data(), 1, p), "history slot", "windows head outside 0..7");
    }
    for (int b : {0, 9, -1}) {
        std::vector<int> nn{1, b};
        expect(windows(p, p, N, R, 1024, 2, rows.data(), fronts.data(), heads.data(), nn.data(), 1, p), "new windows", "windows n_new outside 1..8");
    }
    std::vector<int> f0{3, 5}, nn0{1, 4}, one{1, 1}, fneg{3, -1};
    expect(windows(p, nullptr, N, R, 1024, 2, rows.data(), f0.data(), nullptr, nn0.data(), 0, p), "without attention", "windows att = 0, n_new = 4");
    expect(windows(p, nullptr, N, R, 1024, 2, rows.data(), fneg.data(), nullptr, one.data(), 0, p), "front", "windows att = 0, front = -1");

    // mf_nerf_feat_rows_load: a pool of N = 3 rows as ONE host array with a fourth (scratch) row behind them, so that the overlap checks meet real addresses
    const int dim = 44, ring_row = R * dim, hist_row = 8 * dim * 16;
    alignas(16) static float rings[4 * 32 * 44], hist[4 * 8 * 44 * 16];
    auto load = [&](float* rg, float* hs, int n, int r, int d, int S, const int* rw, const float* sr, const float* sh) {
        return mf_nerf_feat_rows_load(rg, hs, n, r, d, S, rw, sr, sh, nullptr);
    };
    const float *sr = rings + 3 * ring_row, *sh = hist + 3 * hist_row;
    expect(load(nullptr, hist, N, R, dim, 2, rows.data(), sr, sh), "null", "rows_load rings = NULL");
    expect(load(rings, hist, N, R, dim, 2, nullptr, sr, sh), "null", "rows_load rows = NULL");
    expect(load(rings, nullptr, N, R, dim, 2, rows.data(), sr, sh), "null history", "rows_load src_hist without hist");
    for (int d : {0, -1, 1025, 1 << 30}) expect(load(rings, hist, N, R, d, 2, rows.data(), sr, sh), "dim", "rows_load dim outside 1..1024");
    for (int r : {15, 0, -32, 1 << 30, 18}) expect(load(rings, hist, N, r, dim, 2, rows.data(), sr, sh), "ring", "rows_load R outside 16..65536 or no 4 * m");
    for (int n : {0, -1, 1 << 30}) expect(load(rings, hist, n, R, dim, 2, rows.data(), sr, sh), "pool", "rows_load N outside 1..65536");
    for (int S : {0, -2, 4, 1 << 30}) expect(load(rings, hist, N, R, dim, S, rows.data(), sr, sh), "picked", "rows_load n_rows outside 1..N (2 readable)");
    for (int b : {-1, 3, 1 << 30}) {
        std::vector<int> r{0, b};
        expect(load(rings, hist, N, R, dim, 2, r.data(), sr, sh), "out of range", "rows_load row outside the pool");
    }
    expect(load(rings, hist, N, R, dim, 2, twice.data(), sr, sh), "twice", "rows_load a row twice");
    expect(load(rings + 1, hist, N, R, dim, 2, rows.data(), sr, sh), "aligned", "rows_load rings off a 16-byte boundary");
    expect(load(rings, hist, N, R, dim, 2, rows.data(), sr + 2, sh), "aligned", "rows_load src_ring off a 16-byte boundary");
    expect(load(rings, hist, N, R, dim, 2, rows.data(), rings + 2 * ring_row, sh), "ring source overlaps", "rows_load src_ring is named row 2");
    expect(load(rings, hist, N, R, dim, 2, rows.data(), rings + 2 * ring_row - 4, sh), "ring source overlaps", "rows_load src_ring ends inside row 2");
    expect(load(rings, hist, N, R, dim, 2, rows.data(), rings + ring_row - 4, sh), "ring source overlaps", "rows_load src_ring starts inside row 0");
    expect(load(rings, hist, N, R, dim, 2, rows.data(), sr, hist), "history source overlaps", "rows_load src_hist is named row 0");
    expect(load(rings, hist, N, R, dim, 2, rows.data(), sr, hist + 3 * hist_row - 4), "history source overlaps", "rows_load src_hist starts inside row 2");
    std::printf(failures ? "%d FAILED\n" : "all refused as expected (%d failures)\n", failures);
    return failures ? 1 : 0;
}
