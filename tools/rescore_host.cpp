// The body of csrc/rescore.hip (K34) as a plain host program: the table lookups, the back-off walk and the ranking rule are the kernel's
// own functions (RESCORE_HOST_EMU); the wave's part is restated over 64 lanes in a loop -- the two ballots of the segmentation, lane k
// taking words k, k + 64, ..., the butterfly that adds the 64 partial sums.  For checking everything that is indexed by data (table
// slots, pool offsets, word bounds, ranks) without a GPU, and under -fsanitize=address,undefined (a stand-alone binary, nothing
// preloaded): every buffer is allocated at exactly the size the launcher is told, so a stray index is a heap overflow.
//
//   c++ -O1 -std=c++17 [-fsanitize=address,undefined] -Ivoice100_amd/csrc tools/rescore_host.cpp -o rescore_host
//   rescore_host IN OUT      IN: int32 count, then per case int32 {B, nbest, T, order, has_bos, has_eos, use_eos, pool_len, wtab_len,
//                            ng_len}, int64 sep, float64 lm_weight, word_bonus, int64 meta[2 order], pool[pool_len], int32 wtab[wtab_len],
//                            ng[ng_len], int64 ids[B nbest T], int32 lens[B nbest], float32 first[B nbest]
//                            OUT: per case int32 order, n_words, n_oov, lens [B nbest] each, float32 scores, first, lm [B nbest] each,
//                            int64 ids [B nbest T] (tools/rescore_host.py compares them with the oracle)
//   rescore_host --adversarial   a small model whose tables are then damaged: capacities of 1, pool offsets and lengths past the pool,
//                                full tables without an empty slot, slots of garbage; every run must end, stay inside its buffers and
//                                rank every hypothesis exactly once; exits 0
#define RESCORE_HOST_EMU
#include <cstdio>
#include <cstdlib>
#include <string_view>
#include <vector>

#include "rescore.hip"

struct Case {
    int B, nbest, T, use_eos;
    long long sep;
    double alpha, beta;
    RsModel M;
    std::vector<long long> pool, ids;
    std::vector<int> wtab, ng, lens;
    std::vector<float> first;
};
struct Result {
    std::vector<int> order, nw, oov, lens;
    std::vector<float> scores, first, lm;
    std::vector<long long> ids;
};

// rs_segment over a loop of lanes: the same ballots, the same prefix counts
static int segment(const long long* x, int n, long long sep, std::vector<unsigned short>& st, std::vector<unsigned short>& en) {
    int ns = 0, ne = 0;
    for (int p0 = 0; p0 < n; p0 += 64) {
        rs_u64 ms = 0, me = 0;
        for (int lane = 0; lane < 64; ++lane) {
            const int p = p0 + lane;
            const bool in = p < n;
            const long long c = in ? x[p] : sep;
            const long long pv = (in && p > 0) ? x[p - 1] : sep;
            const long long nx = (p + 1 < n) ? x[p + 1] : sep;
            const bool tk = in && c != sep;
            if (tk && pv == sep) ms |= 1ull << lane;
            if (tk && nx == sep) me |= 1ull << lane;
        }
        for (int lane = 0; lane < 64; ++lane) {
            const rs_u64 below = (1ull << lane) - 1ull;
            if (ms >> lane & 1) st.at(ns + __builtin_popcountll(ms & below)) = (unsigned short)(p0 + lane);
            if (me >> lane & 1) en.at(ne + __builtin_popcountll(me & below)) = (unsigned short)(p0 + lane);
        }
        ns += __builtin_popcountll(ms);
        ne += __builtin_popcountll(me);
    }
    return ns;
}

static bool run(const Case& c, Result* out) {
    if (!rs_shape_ok(c.B, c.nbest, c.T) || !rs_model_ok(c.M, (long long)c.wtab.size(), (long long)c.ng.size())) return false;
    if ((size_t)c.M.pool_len != c.pool.size()) return false;
    const int rows = c.B * c.nbest, WM = rs_words_max(c.T);
    out->order.assign(rows, -1); out->nw.assign(rows, -1); out->oov.assign(rows, -1); out->lens.assign(rows, -1);
    out->scores.assign(rows, 0.f); out->first.assign(rows, 0.f); out->lm.assign(rows, 0.f);
    out->ids.assign((size_t)rows * c.T, -1);
    for (int b = 0; b < c.B; ++b) {
        std::vector<double> key(c.nbest), lmv(c.nbest);
        std::vector<int> nwv(c.nbest), oovv(c.nbest), present(c.nbest), rank(c.nbest);
        for (int j = 0; j < c.nbest; ++j) {
            const size_t row = (size_t)b * c.nbest + j;
            const float f = c.first[row];
            present[j] = f > -INFINITY ? 1 : 0;
            double lm = 0.0;
            int nw = 0, oov = 0;
            if (present[j]) {
                std::vector<int> wid(WM);                // the wave's scratch, at its workspace size
                std::vector<unsigned short> st(WM), en(WM);
                int n = c.lens[row];
                n = n < 0 ? 0 : (n > c.T ? c.T : n);
                std::vector<long long> x(c.ids.begin() + row * c.T, c.ids.begin() + row * c.T + n);      // exactly the labels: nothing beyond is read
                nw = segment(x.data(), n, c.sep, st, en);
                for (int k = 0; k < nw; ++k) {
                    const int s0 = st[k] < n - 1 ? st[k] : n - 1;
                    int len = (int)en[k] - s0 + 1;
                    len = len < 1 ? 1 : (len > n - s0 ? n - s0 : len);
                    wid[k] = rs_word_id(c.M, c.pool.data(), c.wtab.data(), x.data() + s0, len);
                    oov += wid[k] == RS_UNK;
                }
                double part[64] = {};
                for (int lane = 0; lane < 64; ++lane)
                    for (int k = lane; k < nw; k += 64) part[lane] += rs_term(c.M, c.ng.data(), wid.data(), k, wid[k]);
                for (int off = 32; off > 0; off >>= 1) {
                    double nxt[64];
                    for (int lane = 0; lane < 64; ++lane) nxt[lane] = part[lane] + part[lane ^ off];
                    for (int lane = 0; lane < 64; ++lane) part[lane] = nxt[lane];
                }
                lm = part[0];
                if (c.use_eos && c.M.has_eos) lm += rs_term(c.M, c.ng.data(), wid.data(), nw, RS_EOS);
            }
            lmv[j] = lm; nwv[j] = nw; oovv[j] = oov;
            key[j] = present[j] ? rs_sort_key(f, c.alpha, lm, c.beta, nw) : -INFINITY;
        }
        for (int j = 0; j < c.nbest; ++j) {
            int r = 0;
            for (int i = 0; i < c.nbest; ++i)
                if (i != j && rs_ahead(key[i], present[i], i, key[j], present[j], j)) ++r;
            rank[j] = r;
            const size_t o = (size_t)b * c.nbest + r, row = (size_t)b * c.nbest + j;
            if (out->order.at(o) != -1) { std::printf("rank %d of utterance %d is taken twice\n", r, b); return false; }
            out->order[o] = j; out->lens[o] = c.lens[row]; out->first[o] = c.first[row];
            out->scores[o] = present[j] ? (float)key[j] : -INFINITY;
            out->lm[o] = (float)lmv[j]; out->nw[o] = nwv[j]; out->oov[o] = oovv[j];
            for (int p = 0; p < c.T; ++p) out->ids.at(o * c.T + p) = c.ids[row * c.T + p];
        }
    }
    return true;
}

// ---- damaged tables ---------------------------------------------------------------------------------------------------------------------
static rs_u64 hash_of(int count, const std::vector<long long>& v) {
    rs_u64 h = (rs_u64)count * 0xD6E8FEB86659FD93ull;
    for (long long x : v) h = rs_mix(h, (rs_u64)x);
    return h;
}

static Case small_case() {                               // words {2 3}, {4}, {5 6 7}: ids 3, 4, 5; order 2; <s> and </s>
    Case c;
    c.B = 2; c.nbest = 5; c.T = 70; c.use_eos = 1; c.sep = 1; c.alpha = 0.5; c.beta = 0.1;
    const std::vector<std::vector<long long>> words = {{2, 3}, {4}, {5, 6, 7}};
    c.wtab.assign(4 * 8, 0);
    for (int s = 0; s < 8; ++s) c.wtab[4 * s] = -1;
    int off = 0;
    for (size_t w = 0; w < words.size(); ++w) {
        unsigned slot = rs_fold(hash_of((int)words[w].size(), words[w])) & 7u;
        while (c.wtab[4 * slot] >= 0) slot = (slot + 1) & 7u;
        c.wtab[4 * slot] = 3 + (int)w; c.wtab[4 * slot + 1] = off; c.wtab[4 * slot + 2] = (int)words[w].size();
        for (long long x : words[w]) c.pool.push_back(x);
        off += (int)words[w].size();
    }
    RsModel& M = c.M;
    M = RsModel{};
    M.order = 2; M.has_bos = 1; M.has_eos = 1; M.pool_len = (int)c.pool.size(); M.wcap = 8;
    M.ng_off[0] = 0; M.ng_cap[0] = 8; M.ng_off[1] = 8 * 3; M.ng_cap[1] = 16;
    c.ng.assign(8 * 3 + 16 * 4, 0);
    for (int s = 0; s < 8; ++s) c.ng[3 * s] = -1;
    for (int s = 0; s < 16; ++s) c.ng[24 + 4 * s] = -1;
    auto put = [&](std::vector<long long> key, float lp, float bow) {
        const int n = (int)key.size(), cap = M.ng_cap[n - 1];
        int* base = c.ng.data() + M.ng_off[n - 1];
        unsigned slot = rs_fold(hash_of(n, key)) & (unsigned)(cap - 1);
        while (base[slot * (n + 2)] >= 0) slot = (slot + 1) & (unsigned)(cap - 1);
        for (int i = 0; i < n; ++i) base[slot * (n + 2) + i] = (int)key[i];
        memcpy(base + slot * (n + 2) + n, &lp, 4);
        memcpy(base + slot * (n + 2) + n + 1, &bow, 4);
    };
    for (int w = 0; w < 6; ++w) put({w}, -1.0f - 0.25f * w, -0.125f * w);
    put({1, 3}, -0.5f, 0.f); put({3, 4}, -0.75f, 0.f); put({4, 2}, -0.25f, 0.f); put({0, 5}, -1.5f, 0.f);
    c.ids.assign((size_t)c.B * c.nbest * c.T, 1);
    c.lens.assign(c.B * c.nbest, 0);
    c.first.assign(c.B * c.nbest, 0.f);
    const std::vector<std::vector<long long>> hyps = {{2, 3, 1, 4}, {4, 1, 1, 5, 6, 7, 1}, {9, 9, 1, 2, 3}, {}, {5, 6, 7, 1, 2, 3, 1, 4, 1, 8}};
    for (int r = 0; r < c.B * c.nbest; ++r) {
        const auto& h = hyps[r % hyps.size()];
        for (size_t p = 0; p < h.size(); ++p) c.ids[(size_t)r * c.T + p] = h[p];
        c.lens[r] = (int)h.size();
        c.first[r] = -3.0f - 0.5f * (r % c.nbest);
    }
    c.first[c.B * c.nbest - 1] = -INFINITY;
    for (int p = 0; p < c.T; ++p) c.ids[(size_t)4 * c.T + p] = (p % 9 == 8) ? 1 : 2 + p % 5;       // one long row of many words
    c.lens[4] = c.T;
    return c;
}

static bool check(const char* name, const Case& c) {
    Result r;
    if (!run(c, &r)) { std::printf("%s: refused or inconsistent\n", name); return false; }
    for (int b = 0; b < c.B; ++b) {
        std::vector<int> seen(c.nbest, 0);
        for (int k = 0; k < c.nbest; ++k) {
            const int j = r.order[b * c.nbest + k];
            if (j < 0 || j >= c.nbest || seen[j]++) { std::printf("%s: utterance %d is not ranked once each\n", name, b); return false; }
        }
    }
    std::printf("%-64s ok (top of utterance 0: hypothesis %d, lm %.4f, %d words, %d unknown)\n", name, r.order[0], r.lm[0], r.nw[0], r.oov[0]);
    return true;
}

static int adversarial() {
    const Case good = small_case();
    bool ok = check("the small model, intact", good);
    { Case c = good; c.wtab.resize(4); c.M.wcap = 1; ok &= check("word table of capacity 1", c); }
    { Case c = good; c.wtab.assign(4, 0); c.wtab[0] = -1; c.M.wcap = 1; ok &= check("word table of capacity 1, empty", c); }
    { Case c = good; for (int s = 0; s < 8; ++s) { c.wtab[4 * s + 1] += 1000000; } ok &= check("pool offsets past the pool", c); }
    { Case c = good; for (int s = 0; s < 8; ++s) { c.wtab[4 * s + 1] = c.M.pool_len - 1; } ok &= check("spellings that run off the pool's end", c); }
    { Case c = good; for (int s = 0; s < 8; ++s) { c.wtab[4 * s + 1] = -7; c.wtab[4 * s + 2] = 0x7fffffff; } ok &= check("negative offsets, huge lengths", c); }
    { Case c = good; for (int s = 0; s < 8; ++s) if (c.wtab[4 * s] < 0) { c.wtab[4 * s] = 77; c.wtab[4 * s + 1] = 0; c.wtab[4 * s + 2] = 9; }
      ok &= check("a full word table without an empty slot", c); }
    { Case c = good; for (size_t i = 0; i < c.ng.size(); ++i) if (c.ng[i] == -1) c.ng[i] = 0x7ffffff0;
      ok &= check("full n-gram tables without an empty slot", c); }
    { Case c = good; c.M.ng_cap[0] = 1; c.M.ng_cap[1] = 1; ok &= check("n-gram tables of capacity 1", c); }
    { Case c = good; for (size_t i = 0; i < c.ng.size(); ++i) c.ng[i] = (int)(i * 2654435761u); for (auto& v : c.wtab) v = v * 31 + 5;
      ok &= check("tables of garbage", c); }
    { Case c = good; c.M.pool_len = 0; c.pool.clear(); ok &= check("an empty pool under a word table that points into it", c); }
    { Case c = good; c.M.ng_off[1] = (int)c.ng.size(); Result r; const bool refused = !run(c, &r);
      std::printf("%-64s %s\n", "an order's table beyond the buffer", refused ? "refused" : "ACCEPTED"); ok &= refused; }
    return ok ? 0 : 1;
}

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }
template <class T>
static void wr(FILE* f, const std::vector<T>& v) { if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f); }

int main(int argc, char** argv) {
    if (argc == 2 && std::string_view(argv[1]) == "--adversarial") return adversarial();
    if (argc != 3) { std::fprintf(stderr, "usage: rescore_host IN OUT | --adversarial\n"); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::fprintf(stderr, "cannot open the files\n"); return 2; }
    int count = 0;
    if (!rd(in, &count, 1)) return 2;
    for (int i = 0; i < count; ++i) {
        int h[10];
        Case c;
        long long meta[2 * RS_MAX_ORDER];
        if (!rd(in, h, 10) || !rd(in, &c.sep, 1) || !rd(in, &c.alpha, 1) || !rd(in, &c.beta, 1)) return 2;
        c.B = h[0]; c.nbest = h[1]; c.T = h[2]; c.use_eos = h[6];
        c.M = RsModel{};
        c.M.order = h[3]; c.M.has_bos = h[4]; c.M.has_eos = h[5]; c.M.pool_len = h[7];
        if (!rs_shape_ok(c.B, c.nbest, c.T) || c.M.order < 1 || c.M.order > RS_MAX_ORDER || h[7] < 0 || h[8] < 4 || h[9] < 0) return 2;
        c.M.wcap = h[8] / 4;
        if (!rd(in, meta, 2 * (size_t)c.M.order)) return 2;
        for (int n = 0; n < c.M.order; ++n) { c.M.ng_off[n] = (int)meta[n]; c.M.ng_cap[n] = (int)meta[c.M.order + n]; }
        const size_t rows = (size_t)c.B * c.nbest;
        c.pool.resize(h[7]); c.wtab.resize(h[8]); c.ng.resize(h[9]); c.ids.resize(rows * c.T); c.lens.resize(rows); c.first.resize(rows);
        if (!rd(in, c.pool.data(), c.pool.size()) || !rd(in, c.wtab.data(), c.wtab.size()) || !rd(in, c.ng.data(), c.ng.size()) ||
            !rd(in, c.ids.data(), c.ids.size()) || !rd(in, c.lens.data(), rows) || !rd(in, c.first.data(), rows))
            return 2;
        Result r;
        if (!run(c, &r)) { std::fprintf(stderr, "case %d: unsupported arguments\n", i); return 3; }
        wr(out, r.order); wr(out, r.nw); wr(out, r.oov); wr(out, r.lens); wr(out, r.scores); wr(out, r.first); wr(out, r.lm); wr(out, r.ids);
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}
