// The bodies of csrc/mbr.hip (K35) as a stand-alone host program: the hash, the posterior's exponent, the ranking rule and the workspace
// layout are the kernels' own code (MBR_HOST_EMU); the waves' part -- the ballot segmentation, the table's compare-and-swap, the ballot
// trimming, the systolic recurrence, the finaliser's threads -- is restated here as serial loops with the same clamps, the same order of
// the floating-point sums and the same workspace, allocated at exactly v100_nbest_mbr_workspace_bytes so that a sanitizer sees a step
// outside it.
//
//   mbr_host cases.bin results.bin     run the cases that tools/mbr_host.py wrote, write the outputs
//   mbr_host --adversarial             lens beyond T and negative, rows of separators only, ids at the int64 extremes, NaN and +-inf scores,
//                                      each on a workspace poisoned with 0x00, 0xFF and 0x7F: exit 0 if every invariant holds
#define MBR_HOST_EMU
#include "mbr.hip"

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

struct Case {
    int B, N, T, Tr, words;
    long long sep;
    double scale;
    std::vector<long long> ids, ref;
    std::vector<int> lens, ref_len;
    std::vector<float> scores;
};

struct Out {
    std::vector<int> order, ntok, lens, dist, ref_dist, ref_n;
    std::vector<float> scores, risk, post, elen;
    std::vector<long long> ids;
};

struct Ws {
    int* tok;
    unsigned* tab;
    int* cnt;
    u16 *st, *en;
};
static Ws ws_of(unsigned char* ws, int b, int R, int W, int P) {
    unsigned char* base = ws + (size_t)b * mb_ws_per(R, W);
    Ws w;
    w.tok = (int*)base;
    w.tab = (unsigned*)(w.tok + (size_t)R * W);
    w.cnt = (int*)(w.tab + P);
    w.st = (u16*)(w.cnt + MB_ROWS_MAX + 3);
    w.en = w.st + (size_t)R * W;
    return w;
}

static int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// mb_segment without the ballots: the k-th run start and the k-th run end are word k
static int segment(const long long* x, int n, long long sep, u16* st, u16* en) {
    int ns = 0, ne = 0;
    for (int p = 0; p < n; ++p) {
        const long long c = x[p], pv = p > 0 ? x[p - 1] : sep, nx = p + 1 < n ? x[p + 1] : sep;
        if (c != sep && pv == sep) st[ns++] = (u16)p;
        if (c != sep && nx == sep) en[ne++] = (u16)p;
    }
    return ns;
}

static void tokenise(const Case& c, unsigned char* ws, int b, int P) {
    const int N = c.N, T = c.T, Tr = c.Tr, R = mb_rows(N, Tr), W = mb_width(T, Tr);
    const Ws w = ws_of(ws, b, R, W, P);
    int s_len[MB_ROWS_MAX], s_cnt[MB_ROWS_MAX];
    auto row_ptr = [&](int r) { return r < N ? c.ids.data() + ((size_t)b * N + r) * T : c.ref.data() + (size_t)b * Tr; };
    for (int i = 0; i < P; ++i) w.tab[i] = MB_EMPTY;
    for (int r = 0; r < R; ++r) {
        int n = 0;
        if (r == N) n = clampi(c.ref_len[b], 0, Tr);
        else if (mb_present(c.scores[(size_t)b * N + r])) n = clampi(c.lens[(size_t)b * N + r], 0, T);
        int cnt = n;
        if (c.words) cnt = segment(row_ptr(r), n, c.sep, w.st + (size_t)r * W, w.en + (size_t)r * W);
        s_len[r] = n;
        s_cnt[r] = cnt;
        w.cnt[r] = cnt;
    }
    auto token = [&](int r, int k, const long long*& p, int& len) {
        const int n = s_len[r];
        int s0 = k;
        len = 1;
        if (c.words) {
            s0 = std::min((int)w.st[(size_t)r * W + k], n - 1);
            len = std::min(std::max((int)w.en[(size_t)r * W + k] - s0 + 1, 1), n - s0);
        }
        p = row_ptr(r) + s0;
    };
    const unsigned mask = (unsigned)P - 1u;
    for (int r = 0; r < R; ++r)
        for (int k = 0; k < s_cnt[r]; ++k) {
            const long long* p;
            int len;
            token(r, k, p, len);
            const unsigned self = (unsigned)(r * W + k);
            unsigned slot = mb_fold(mb_hash(p, len)) & mask;
            int id = (int)self;
            for (int probe = 0; probe < P; ++probe) {
                const unsigned cur = w.tab[slot];        // atomicCAS(&tab[slot], MB_EMPTY, self), one token at a time
                if (cur == MB_EMPTY) {
                    w.tab[slot] = self;
                    break;
                }
                const int r2 = (int)(cur / (unsigned)W), k2 = (int)(cur % (unsigned)W);
                if (r2 < R && k2 < s_cnt[r2]) {
                    const long long* q;
                    int qlen;
                    token(r2, k2, q, qlen);
                    bool same = qlen == len;
                    for (int i = 0; same && i < len; ++i) same = q[i] == p[i];
                    if (same) {
                        id = (int)cur;
                        break;
                    }
                }
                slot = (slot + 1) & mask;
            }
            w.tok[(size_t)r * W + k] = id;
        }
}

// D[nr][mc] of rows[0 .. nr) against cols[0 .. mc): what mb_systolic computes, one row after the other
static int recurrence(const int* cols, const int* rows, int mc, int nr) {
    std::vector<int> d(mc + 1);
    for (int j = 0; j <= mc; ++j) d[j] = j;
    for (int i = 1; i <= nr; ++i) {
        int diag = d[0];
        d[0] = i;
        for (int j = 1; j <= mc; ++j) {
            const int up = d[j];
            d[j] = std::min(std::min(up + 1, diag + (cols[j - 1] != rows[i - 1] ? 1 : 0)), d[j - 1] + 1);
            diag = up;
        }
    }
    return d[mc];
}

static void pairs(const Case& c, unsigned char* ws, int b, int P, Out& o) {
    const int N = c.N, R = mb_rows(N, c.Tr), W = mb_width(c.T, c.Tr);
    const Ws w = ws_of(ws, b, R, W, P);
    const int NP = N * (N - 1) / 2, total = NP + (c.Tr > 0 ? N : 0);
    for (int q0 = 0; q0 < total; ++q0) {
        int q = q0, i, j;
        if (q < NP) {
            i = 0;
            while (q >= N - 1 - i) {
                q -= N - 1 - i;
                ++i;
            }
            j = i + 1 + q;
        } else {
            i = q - NP;
            j = N;
        }
        int* d_ij = j < N ? &o.dist[((size_t)b * N + i) * N + j] : &o.ref_dist[(size_t)b * N + i];
        int* d_ji = j < N ? &o.dist[((size_t)b * N + j) * N + i] : d_ij;
        int both = mb_present(c.scores[(size_t)b * N + i]);
        if (j < N) both &= mb_present(c.scores[(size_t)b * N + j]);
        if (!both) {
            *d_ij = *d_ji = -1;
            continue;
        }
        const int n = clampi(w.cnt[i], 0, W), m = clampi(w.cnt[j], 0, W);
        const int* a = w.tok + (size_t)i * W;
        const int* cc = w.tok + (size_t)j * W;
        const int mn = std::min(n, m);
        int p = 0;
        while (p < mn && a[p] == cc[p]) ++p;
        const int lim = mn - p;                          // the suffix may not reach into the prefix
        int s = 0;
        while (s < lim && a[n - 1 - s] == cc[m - 1 - s]) ++s;
        const int na = n - p - s, nc = m - p - s;
        const bool swap = na < nc;
        const int* cols = (swap ? a : cc) + p;
        const int* rows = (swap ? cc : a) + p;
        const int mc = swap ? na : nc, nr = swap ? nc : na;
        *d_ij = *d_ji = mc == 0 ? nr : recurrence(cols, rows, mc, nr);
    }
}

static void finalise(const Case& c, unsigned char* ws, int b, int P, Out& o) {
    const int N = c.N, T = c.T, R = mb_rows(N, c.Tr), W = mb_width(T, c.Tr);
    const Ws w = ws_of(ws, b, R, W, P);
    const size_t row0 = (size_t)b * N;
    double s_e[MB_NBEST_MAX], s_p[MB_NBEST_MAX];
    float s_f[MB_NBEST_MAX], s_risk[MB_NBEST_MAX];
    int s_present[MB_NBEST_MAX], s_nt[MB_NBEST_MAX];
    for (int i = 0; i < N; ++i) {
        s_f[i] = c.scores[row0 + i];
        s_present[i] = mb_present(s_f[i]);
        s_nt[i] = s_present[i] ? clampi(w.cnt[i], 0, W) : 0;
    }
    float s_max = -INFINITY;
    for (int j = 0; j < N; ++j)
        if (s_present[j]) s_max = fmaxf(s_max, s_f[j]);
    double z = 0.0;
    for (int i = 0; i < N; ++i) {
        s_e[i] = s_present[i] ? exp(mb_arg(c.scale, s_f[i], s_max)) : 0.0;
        z += s_e[i];
    }
    for (int i = 0; i < N; ++i) s_p[i] = z > 0.0 ? s_e[i] / z : 0.0;
    for (int i = 0; i < N; ++i) {
        double risk = 0.0;
        for (int j = 0; j < N; ++j)
            if (j != i && s_present[j]) risk = risk + s_p[j] * (double)o.dist[(row0 + i) * N + j];
        s_risk[i] = s_present[i] ? (float)risk : INFINITY;
        o.dist[(row0 + i) * N + i] = s_present[i] ? 0 : -1;
    }
    double el = 0.0;
    for (int j = 0; j < N; ++j) el = el + s_p[j] * (double)s_nt[j];
    o.elen[b] = (float)el;
    if (c.Tr > 0) o.ref_n[b] = clampi(w.cnt[N], 0, W);
    for (int j = 0; j < N; ++j) {
        int rank = 0;
        for (int i = 0; i < N; ++i)
            if (i != j && mb_ahead(s_risk[i], s_present[i], i, s_risk[j], s_present[j], j)) ++rank;
        const size_t at = row0 + rank;
        o.order[at] = j;
        o.lens[at] = c.lens[row0 + j];
        o.scores[at] = s_f[j];
        o.risk[at] = s_risk[j];
        o.post[at] = (float)s_p[j];
        o.ntok[at] = s_nt[j];
        memcpy(&o.ids[at * T], &c.ids[(row0 + j) * T], sizeof(long long) * T);
    }
}

static bool run(const Case& c, int poison, Out& o) {
    const long long nbytes = mb_shape_ok(c.B, c.N, c.T, c.Tr) ? (long long)c.B * (long long)mb_ws_per(mb_rows(c.N, c.Tr), mb_width(c.T, c.Tr)) : -1;
    if (nbytes <= 0 || !(c.scale - c.scale == 0.0) || c.scale < 0.0) return false;
    unsigned char* ws = (unsigned char*)malloc((size_t)nbytes);
    memset(ws, poison, (size_t)nbytes);
    const size_t BN = (size_t)c.B * c.N;
    o.order.assign(BN, -7), o.ntok.assign(BN, -7), o.lens.assign(BN, -7), o.dist.assign(BN * c.N, -7), o.ref_dist.assign(c.Tr > 0 ? BN : 0, -7);
    o.ref_n.assign(c.Tr > 0 ? c.B : 0, -7), o.scores.assign(BN, 0.f), o.risk.assign(BN, 0.f), o.post.assign(BN, 0.f), o.elen.assign(c.B, 0.f);
    o.ids.assign(BN * c.T, -7);
    const int P = mb_slots(mb_rows(c.N, c.Tr), mb_width(c.T, c.Tr));
    for (int b = 0; b < c.B; ++b) tokenise(c, ws, b, P);
    for (int b = 0; b < c.B; ++b) pairs(c, ws, b, P, o);
    for (int b = 0; b < c.B; ++b) finalise(c, ws, b, P, o);
    free(ws);
    return true;
}

template <class V>
static bool same_bytes(const V& a, const V& b) {
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0);
}
static bool same(const Out& a, const Out& b) {
    return same_bytes(a.order, b.order) && same_bytes(a.ntok, b.ntok) && same_bytes(a.lens, b.lens) && same_bytes(a.dist, b.dist) &&
           same_bytes(a.ref_dist, b.ref_dist) && same_bytes(a.ref_n, b.ref_n) && same_bytes(a.scores, b.scores) && same_bytes(a.risk, b.risk) &&
           same_bytes(a.post, b.post) && same_bytes(a.elen, b.elen) && same_bytes(a.ids, b.ids);
}

#define NEED(x) do { if (!(x)) { fprintf(stderr, "adversarial %d: %s\n", which, #x); return false; } } while (0)

static bool invariants(const Case& c, const Out& o, int which) {
    const int N = c.N;
    for (int b = 0; b < c.B; ++b) {
        std::vector<int> seen(N, 0);
        const size_t row0 = (size_t)b * N;
        bool absent_from = false;
        for (int r = 0; r < N; ++r) {
            const int j = o.order[row0 + r];
            NEED(j >= 0 && j < N && !seen[j]);
            seen[j] = 1;
            const bool here = mb_present(c.scores[row0 + j]);
            NEED(!(absent_from && here));                // the absent ones are behind every present one
            absent_from = absent_from || !here;
            const float risk = o.risk[row0 + r], post = o.post[row0 + r];
            NEED(here ? (risk >= 0.f && risk < INFINITY && post >= 0.f && post <= 1.f) : (risk == INFINITY && post == 0.f && o.ntok[row0 + r] == 0));
            NEED(o.ntok[row0 + r] >= 0 && o.ntok[row0 + r] <= c.T);
            if (r > 0 && here) NEED(o.risk[row0 + r - 1] <= risk);
        }
        NEED(o.elen[b] >= 0.f && o.elen[b] <= (float)c.T);
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j) {
                const int d = o.dist[(row0 + i) * N + j];
                const bool both = mb_present(c.scores[row0 + i]) && mb_present(c.scores[row0 + j]);
                NEED(d == o.dist[(row0 + j) * N + i] && (both ? (i == j ? d == 0 : d >= 0 && d <= c.T) : d == -1));
            }
        if (c.Tr > 0) {
            NEED(o.ref_n[b] >= 0 && o.ref_n[b] <= c.Tr);
            for (int i = 0; i < N; ++i) {
                const int d = o.ref_dist[row0 + i];
                NEED(mb_present(c.scores[row0 + i]) ? (d >= 0 && d <= std::max(c.T, c.Tr)) : d == -1);
            }
        }
    }
    return true;
}

static int adversarial() {
    const long long MAXI = 0x7fffffffffffffffll, MINI = -MAXI - 1;
    const int bad_lens[] = {-1, -2147483647 - 1, 2147483647, 4097, 9, 8, 0, 1 << 30};
    const float bad_scores[] = {-1.f, NAN, INFINITY, -INFINITY, -2.f, 3.0e38f, -3.0e38f, 0.f};
    unsigned seed = 12345u;
    auto next = [&]() { return seed = seed * 1664525u + 1013904223u; };
    int which = 0;
    for (int words = 0; words < 2; ++words)
        for (int shape = 0; shape < 6; ++shape, ++which) {
            Case c;
            c.B = 2, c.N = shape == 5 ? 64 : 8, c.T = shape == 4 ? 1 : 8, c.Tr = (shape & 1) ? 5 : 0, c.words = words;
            c.sep = shape == 2 ? MINI : 1;
            c.scale = shape == 3 ? 0.0 : shape == 2 ? 1.0e300 : 1.0;
            const size_t BN = (size_t)c.B * c.N;
            c.ids.resize(BN * c.T), c.lens.resize(BN), c.scores.resize(BN), c.ref.resize((size_t)c.B * c.Tr), c.ref_len.resize(c.Tr ? c.B : 0);
            for (size_t i = 0; i < c.ids.size(); ++i) {
                const unsigned v = next() >> 24;
                c.ids[i] = v < 80 ? c.sep : v < 110 ? MAXI : v < 140 ? MINI : (long long)(v & 3);
            }
            for (size_t r = 0; r < BN; ++r) {
                c.lens[r] = bad_lens[(r + shape) % 8];
                c.scores[r] = shape == 0 ? bad_scores[r % 8] : (r % 3 ? -0.5f * (float)(r % 5) : bad_scores[(r / 3) % 8]);
                if (r % 8 == 6)
                    for (int p = 0; p < c.T; ++p) c.ids[r * c.T + p] = c.sep;            // a row of separators only
            }
            if (shape == 1)
                for (size_t r = c.N; r < BN; ++r) c.scores[r] = r & 1 ? NAN : -INFINITY;     // an utterance with no hypothesis
            for (size_t i = 0; i < c.ref.size(); ++i) c.ref[i] = (next() >> 28) < 5 ? c.sep : (next() >> 30 ? MAXI : 2);
            for (size_t i = 0; i < c.ref_len.size(); ++i) c.ref_len[i] = i ? -5 : 100000;
            Out first;
            if (!run(c, 0x00, first) || !invariants(c, first, which)) return 1;
            for (int poison : {0xFF, 0x7F}) {
                Out again;
                if (!run(c, poison, again) || !same(first, again)) {
                    fprintf(stderr, "adversarial %d: a workspace of 0x%02X changes the outputs\n", which, poison);
                    return 1;
                }
            }
        }
    Case c;                                              // what the launcher refuses is refused here too
    c.B = 1, c.N = 65, c.T = 4, c.Tr = 0, c.words = 1, c.sep = 1, c.scale = 1.0;
    Out o;
    if (run(c, 0, o)) return 1;
    c.N = 2, c.scale = NAN;
    if (run(c, 0, o)) return 1;
    printf("adversarial: %d inputs on three workspaces each, every invariant holds\n", which);
    return 0;
}

template <class V>
static bool rd(FILE* f, V& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(v[0]), n, f) == n;
}
template <class V>
static void wr(FILE* f, const V& v) {
    if (!v.empty()) fwrite(v.data(), sizeof(v[0]), v.size(), f);
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--adversarial")) return adversarial();
    if (argc != 3) {
        fprintf(stderr, "usage: mbr_host cases.bin results.bin | mbr_host --adversarial\n");
        return 2;
    }
    FILE* fin = fopen(argv[1], "rb");
    FILE* fout = fopen(argv[2], "wb");
    if (!fin || !fout) return 2;
    int n_cases = 0;
    if (fread(&n_cases, 4, 1, fin) != 1) return 2;
    for (int k = 0; k < n_cases; ++k) {
        Case c;
        int head[5];
        if (fread(head, 4, 5, fin) != 5 || fread(&c.sep, 8, 1, fin) != 1 || fread(&c.scale, 8, 1, fin) != 1) return 2;
        c.B = head[0], c.N = head[1], c.T = head[2], c.Tr = head[3], c.words = head[4];
        if (!mb_shape_ok(c.B, c.N, c.T, c.Tr)) return 2;
        const size_t BN = (size_t)c.B * c.N;
        if (!rd(fin, c.ids, BN * c.T) || !rd(fin, c.lens, BN) || !rd(fin, c.scores, BN) || !rd(fin, c.ref, (size_t)c.B * c.Tr) ||
            !rd(fin, c.ref_len, c.Tr ? c.B : 0))
            return 2;
        Out o, again;
        if (!run(c, 0xA5, o) || !run(c, 0xFF, again) || !same(o, again)) {
            fprintf(stderr, "case %d: refused, or the workspace's content changes the outputs\n", k);
            return 1;
        }
        wr(fout, o.order), wr(fout, o.ntok), wr(fout, o.lens), wr(fout, o.scores), wr(fout, o.risk), wr(fout, o.post), wr(fout, o.ids);
        wr(fout, o.dist), wr(fout, o.elen), wr(fout, o.ref_dist), wr(fout, o.ref_n);
    }
    fclose(fin);
    fclose(fout);
    return 0;
}
