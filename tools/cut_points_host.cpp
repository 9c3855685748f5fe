// The walk and the table bodies of csrc/cut_points.hip (K31) as a plain host program: the workgroup's CP_THREADS lanes are host threads,
// its barrier a std::barrier, its block-wide max and scan loops over a shared array.  For checking the data-indexed part of the cutter
// (run tables, cut indices, the piece table) without a GPU, and under -fsanitize=address,undefined (a stand-alone binary, nothing
// preloaded); every table is allocated at exactly the size the workspace gives it, so a stray index is a heap overflow.
//
//   c++ -O1 -std=c++20 -pthread [-fsanitize=address,undefined] -Ivoice100_amd/csrc tools/cut_points_host.cpp -o cut_points_host
//   cut_points_host IN OUT     IN: int32 count, then per case int32 {T, n, max_frames, min_gap (0: none), pad, min_frames}, float32 margin
//                              and float32 margins d[n] as tests/_cut_points_ref.margins gives them (NaN included)
//                              OUT: per case int32 n_seg, then start, end, forced [n_seg] each, then two entries past n_seg
//   cut_points_host --adversarial     built-in rows: all silent, none silent, alternating frames at T = 2^20 with min_gap 1 (the
//                                     largest run table), oversized cores without a silent frame or without stage A at min_frames 1
//                                     (a cut every few frames), NaN and infinite margins; checks the promises on each and exits 0
#define CUT_POINTS_HOST_EMU
#define _USE_MATH_DEFINES
#include <barrier>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string_view>
#include <thread>
#include <vector>

#include "cut_points.hip"

static std::barrier<> g_bar(CP_THREADS);
static cp_u64 g_u64[CP_THREADS];
static int g_int[CP_THREADS];

void cp_sync() { g_bar.arrive_and_wait(); }
cp_u64 cp_block_max(CpShared&, int tid, cp_u64 v) {
    g_u64[tid] = v;
    cp_sync();
    cp_u64 m = 0;
    for (int i = 0; i < CP_THREADS; ++i) m = g_u64[i] > m ? g_u64[i] : m;
    cp_sync();
    return m;
}
int cp_block_scan(CpShared&, int tid, int v, int* total) {
    g_int[tid] = v;
    cp_sync();
    int before = 0, all = 0;
    for (int i = 0; i < CP_THREADS; ++i) { if (i < tid) before += g_int[i]; all += g_int[i]; }
    cp_sync();
    *total = all;
    return before;
}

struct Case { int T, n, max_frames, min_gap, pad, min_frames; float margin; std::vector<float> d; };
struct Table { int n_seg; std::vector<int> start, end, forced; };

static bool run(const Case& c, Table* out) {
    if (!cp_supported(1, c.T, 2, 0, c.max_frames, c.min_gap, c.pad, c.min_frames) || c.n < 0 || c.n > c.T) return false;
    const CpLayout L = cp_layout(c.T);
    // what the frame pass leaves: the margins with NaN as -inf, and the words of silent bits (zero beyond n)
    std::vector<float> d(c.T);
    std::vector<cp_u64> mask(L.words, 0);
    for (int t = 0; t < c.n; ++t) {
        const float v = std::isnan(c.d[t]) ? -INFINITY : c.d[t];
        d[t] = v;
        if (v > c.margin) mask[t / 64] |= 1ull << (t % 64);
    }
    std::vector<int> hdr(4, 0), rs(L.runs), re(L.runs), cut(L.runs), ps(c.T), pe(c.T);
    int n_seg = -1;
    const CpArgs A = {c.T, c.max_frames - 2 * c.pad, c.min_gap, c.min_frames};
    static CpShared S;
    std::vector<std::thread> lanes;
    for (int tid = 0; tid < CP_THREADS; ++tid)
        lanes.emplace_back([&, tid] { cp_walk(S, tid, A, c.n, d.data(), mask.data(), hdr.data(), rs.data(), re.data(), cut.data(), ps.data(), pe.data(), L.runs, &n_seg); });
    for (auto& t : lanes) t.join();
    out->n_seg = n_seg;
    const int rows = n_seg + 2;
    out->start.assign(rows, -1); out->end.assign(rows, -1); out->forced.assign(rows, -1);
    for (int k = 0; k < rows; ++k) cp_table_entry(hdr.data(), ps.data(), pe.data(), k, c.pad, &out->start[k], &out->end[k], &out->forced[k]);
    return true;
}

// the promises that need no reference: order, bounds, lengths, every non-silent frame covered once, zeros past the end
static bool promises(const Case& c, const Table& t, const char* name) {
    int prev = 0, loud = 0, covered = 0;
    for (int k = 0; k < t.n_seg; ++k) {
        if (!(t.start[k] >= prev && t.end[k] > t.start[k] && t.end[k] <= c.n && t.end[k] - t.start[k] <= c.max_frames)) {
            std::printf("%s: segment %d = [%d, %d) breaks a promise\n", name, k, t.start[k], t.end[k]);
            return false;
        }
        if (t.forced[k] && (k == 0 || t.start[k] != t.end[k - 1])) { std::printf("%s: forced segment %d\n", name, k); return false; }
        for (int f = t.start[k]; f < t.end[k]; ++f) covered += !(c.d[f] > c.margin);
        prev = t.end[k];
    }
    for (int f = 0; f < c.n; ++f) loud += !(c.d[f] > c.margin);
    for (int k = t.n_seg; k < t.n_seg + 2; ++k)
        if (t.start[k] || t.end[k] || t.forced[k]) { std::printf("%s: entry %d past the end is not zero\n", name, k); return false; }
    if (loud != covered) { std::printf("%s: %d of %d non-silent frames covered\n", name, covered, loud); return false; }
    std::printf("%-58s n %8d  segments %7d\n", name, c.n, t.n_seg);
    return true;
}

static int adversarial() {
    std::vector<std::pair<const char*, Case>> cases;
    auto flat = [](int T, float v) { return std::vector<float>(T, v); };
    cases.push_back({"all silent", {5000, 5000, 3000, 25, 5, 50, 0.0f, flat(5000, 3.0f)}});
    cases.push_back({"none silent, forced all the way, min_frames 1", {7001, 7001, 4, 1, 0, 1, 0.0f, flat(7001, -3.0f)}});
    cases.push_back({"none silent, all margins NaN", {9000, 8999, 16, 3, 2, 4, 0.0f, flat(9000, NAN)}});
    { Case c{1 << 20, 1 << 20, 3000, 1, 5, 50, 0.0f, flat(1 << 20, -1.0f)};
      for (int t = 1; t < c.T; t += 2) c.d[t] = 1.0f;
      cases.push_back({"alternating frames at 2^20, min_gap 1", c}); }
    { Case c{20001, 20000, 8, 0, 0, 1, 0.0f, flat(20001, -1.0f)};
      for (int t = 1; t < c.T; t += 2) c.d[t] = 1.0f;
      cases.push_back({"alternating frames, no stage A, max_frames 8", c}); }
    { Case c{40000, 40000, 64, 25, 5, 8, 0.5f, flat(40000, -INFINITY)};
      for (int t = 0; t < c.T; ++t) c.d[t] = (t % 97 < 3) ? INFINITY : ((t % 31 == 0) ? NAN : ((t % 7 == 0) ? 0.5f : -INFINITY));
      cases.push_back({"infinite and NaN margins, margin 0.5", c}); }
    { Case c{65, 65, 8, 2, 1, 2, 0.0f, flat(65, 1.0f)};
      c.d[0] = -1.0f; c.d[64] = -1.0f;
      cases.push_back({"one non-silent frame at each end", c}); }
    for (auto& [name, c] : cases) {
        Table t;
        if (!run(c, &t) || !promises(c, t, name)) return 1;
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && std::string_view(argv[1]) == "--adversarial") return adversarial();
    if (argc != 3) { std::fprintf(stderr, "usage: cut_points_host IN OUT | --adversarial\n"); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::fprintf(stderr, "cannot open the files\n"); return 2; }
    int count = 0;
    if (std::fread(&count, 4, 1, in) != 1) return 2;
    for (int i = 0; i < count; ++i) {
        int h[6];
        Case c;
        if (std::fread(h, 4, 6, in) != 6 || std::fread(&c.margin, 4, 1, in) != 1) return 2;
        c.T = h[0]; c.n = h[1]; c.max_frames = h[2]; c.min_gap = h[3]; c.pad = h[4]; c.min_frames = h[5];
        if (c.T < 1 || c.T > CP_TMAX || c.n < 0 || c.n > c.T) return 2;
        c.d.assign(c.T, 0.0f);
        if (c.n && std::fread(c.d.data(), 4, c.n, in) != (size_t)c.n) return 2;
        Table t;
        if (!run(c, &t)) { std::fprintf(stderr, "case %d: unsupported arguments\n", i); return 3; }
        std::fwrite(&t.n_seg, 4, 1, out);
        std::fwrite(t.start.data(), 4, t.n_seg, out);
        std::fwrite(t.end.data(), 4, t.n_seg, out);
        std::fwrite(t.forced.data(), 4, t.n_seg, out);
        std::fwrite(t.start.data() + t.n_seg, 4, 2, out);
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}
