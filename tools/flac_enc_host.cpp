// The per-lane bodies of csrc/flac_enc.hip (K30) as a plain host program: every phase of every workgroup runs as a loop over its threads.
// For checking the encoder's logic without a GPU, and under -fsanitize=address,undefined (a stand-alone binary, nothing preloaded):
//
//   c++ -O1 -std=c++17 -ffp-contract=off [-fsanitize=address,undefined] -Ivoice100_amd/csrc tools/flac_enc_host.cpp -o flac_enc_host
//   flac_enc_host IN OUT     IN: cases, each 10 int32 {channels, samples, bits, block size, max LPC order, max partition order,
//                            rate code, rate trailer, float input (0/1), 0} then [channels][samples] int32 or float32
//                            OUT: per case int64 status code, int64 status sample, int64 bytes, then the frames
//   flac_enc_host --adversarial     built-in PCM that stresses the arithmetic: all-minimum samples, alternating extremes at 24 bits,
//                                   length 1; prints the sizes and exits 0
#define FLAC_ENC_HOST_EMU
#include "flac_enc.hip"

#include <cstdio>
#include <cstdlib>
#include <string_view>
#include <vector>

struct Result { int code, where; std::vector<unsigned char> bytes; };

static Result encode(const std::vector<int>& pcm, const std::vector<float>& wave, int C, int n, int bps, int bs, int max_lpc, int max_po,
                     int rate_code, int rate_extra) {
    static FeAnalyze SA;
    static FeLayout SL;
    static FePack SP;
    static FeCrc SC;
    const int F = (n + bs - 1) / bs, nsig = C == 1 ? 1 : 4;
    FeArgs a;
    a.xf = wave.empty() ? nullptr : wave.data(); a.xi = wave.empty() ? pcm.data() : nullptr; a.N = n; a.R = 1; a.C = C; a.bps = bps;
    a.block_size = bs; a.max_lpc = max_lpc; a.max_po = max_po; a.B = 1; a.F = F; a.rate_code = rate_code; a.rate_extra = rate_extra;
    Result r{0, 0, {}};
    FeWs w;
    if (!fe_ws_layout(F, C, &w) || !fe_args_ok(a)) { r.code = -1; return r; }
    std::vector<int> ftab((size_t)F * FE_FTAB, 0), plan((size_t)F * nsig * FE_PLAN, 0), frec((size_t)F * 4, 0), report(F, 0), status(2, 0);
    std::vector<long long> foff(F, 0);
    for (int f = 0; f < F; ++f) {
        int* fr = &ftab[(size_t)f * FE_FTAB];
        fr[FF_ROW] = 0; fr[FF_START] = f * bs; fr[FF_N] = n - f * bs < bs ? n - f * bs : bs; fr[FF_NUM] = f; fr[FF_ITEM] = 0;
    }
    long long cap = 0;
    for (int f = 0; f < F; ++f) cap += 16 + (16 + (long long)(C * bps + (C == 2)) * ftab[(size_t)f * FE_FTAB + FF_N] + 7) / 8 + 2;
    cap = (cap + 3) / 4 * 4;
    std::vector<unsigned char> out((size_t)cap, 0);
    for (int f = 0; f < F; ++f)
        for (int s = 0; s < nsig; ++s)
            fe_analyze(SA, a, &ftab[(size_t)f * FE_FTAB], s, status.data(), &plan[((size_t)f * nsig + s) * FE_PLAN]);
    fe_layout(SL, a, ftab.data(), plan.data(), frec.data(), foff.data(), report.data());
    for (int f = 0; f < F; ++f)
        fe_pack(SP, a, &ftab[(size_t)f * FE_FTAB], &plan[(size_t)f * nsig * FE_PLAN], &frec[(size_t)f * 4], foff[f], out.data(), cap, status.data());
    for (int f = 0; f < F; ++f) fe_crc(SC, &frec[(size_t)f * 4], foff[f], out.data(), cap);
    long long total = 0;
    for (int f = 0; f < F; ++f) total += report[f];
    r.code = status[0];
    r.where = status[0] ? 0x7FFFFFFF - status[1] : 0;
    r.bytes.assign(out.begin(), out.begin() + total);
    return r;
}

static int adversarial() {
    struct Case { const char* name; int alternate, C, n, bps, bs, lpc; };
    const Case cases[] = {{"all-minimum 16-bit", 0, 1, 5000, 16, 4096, 12}, {"all-minimum 24-bit stereo", 0, 2, 600, 24, 192, 12},
                          {"alternating extremes 24-bit", 1, 1, 4608, 24, 4608, 12}, {"alternating extremes 24-bit stereo, inverted", 1, 2, 1153, 24, 1152, 12},
                          {"alternating extremes 8-bit", 1, 1, 33, 8, 16, 8}, {"length 1", 0, 1, 1, 16, 4096, 8}, {"length 1 stereo 24-bit", 0, 2, 1, 24, 16, 12}};
    for (const Case& c : cases) {
        std::vector<int> pcm((size_t)c.C * c.n);
        const int hi = (1 << (c.bps - 1)) - 1, lo = -hi - 1;
        for (int ch = 0; ch < c.C; ++ch)
            for (int i = 0; i < c.n; ++i) {
                int v = lo;
                if (c.alternate) v = ((i + ch) & 1) ? hi : lo;
                if (c.n == 1) v = ch ? hi : lo;
                pcm[(size_t)ch * c.n + i] = v;
            }
        const Result r = encode(pcm, {}, c.C, c.n, c.bps, c.bs, c.lpc, 6, 5, 0);
        std::printf("%-46s status %d, %zu bytes\n", c.name, r.code, r.bytes.size());
        if (r.code || r.bytes.empty()) return 1;
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && std::string_view(argv[1]) == "--adversarial") return adversarial();
    if (argc != 3) { std::fprintf(stderr, "usage: %s IN OUT | --adversarial\n", argv[0]); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::fprintf(stderr, "cannot open the files\n"); return 2; }
    int h[10];
    while (std::fread(h, sizeof(int), 10, in) == 10) {
        const int C = h[0], n = h[1];
        if (C < 1 || C > 2 || n < 1 || n > (1 << 24)) return 2;
        std::vector<int> pcm;
        std::vector<float> wave;
        const size_t cnt = (size_t)C * n;
        if (h[8]) { wave.resize(cnt); if (std::fread(wave.data(), 4, cnt, in) != cnt) return 2; }
        else { pcm.resize(cnt); if (std::fread(pcm.data(), 4, cnt, in) != cnt) return 2; }
        const Result r = encode(pcm, wave, C, n, h[2], h[3], h[4], h[5], h[6], h[7]);
        const long long head[3] = {r.code, r.where, (long long)r.bytes.size()};
        std::fwrite(head, 8, 3, out);
        std::fwrite(r.bytes.data(), 1, r.bytes.size(), out);
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}
