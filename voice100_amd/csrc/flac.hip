// K28: FLAC (LibriSpeech's container) decoded on the device, a batch of files per call, four launches.
//
//   a. flac_scan_kernel    one thread per byte offset: a frame header that is well formed, passes its CRC-8 and agrees with the file's
//                          STREAMINFO is a CANDIDATE.  Candidates take a slot from a per-file atomic counter and enter a per-file
//                          open-addressing table keyed by their offset (64-bit compare-and-swap, load <= 1/2).  More candidates than
//                          slots is a status, never a write.
//   b. flac_decode_kernel  one LANE per candidate, 64 candidates a wave: every candidate is decoded speculatively into its slot's
//                          staging area, with its end offset and whether its CRC-16 matched.
//   c. flac_chain_kernel   one thread per file walks the chain from the first frame: each frame's CRC-16 matched, the next begins where
//                          it ended, the sample positions are consecutive, and the chain ends at the file's end with total_samples.
//                          Candidates off the chain are never looked at; a break is a status with the frame index.
//   d. flac_commit_kernel  one workgroup per accepted slot: wasted bits restored, stereo decorrelation undone, int32 PCM and
//                          float32 (int / 2^(bps-1)) rows written, whole lines per wave instruction on both sides.
//
// The decode lane.  The sample loop is the same for every lane whatever its subframe type: constant is a fixed predictor of order 1
// with zero-bit raw residuals, verbatim an order-0 predictor with raw residuals of the sample width, a fixed predictor an LPC with
// the binomial coefficients and shift 0, and every predictor runs the wave's LARGEST order with zero coefficients above its own.
// The loop counter i is wave-uniform, so the history ring's slot (i & 31) is too: ring and coefficients live in LDS as [tap][lane],
// 64 lanes on 64 consecutive dwords.  Bits come from a 64-bit window, refilled by one byte-swapped dword load issued a refill ahead
// of its use (16-byte loads four dwords ahead were tried and measured no faster); a unary run is a clz on the window.  Every load is clamped to the file's padded end and every position is checked
// against the file's end, so garbage in is a status out.  Every 16 samples the wave transposes its last 16 ring rows through LDS
// into the staging areas, 64-byte segments per frame (flac_flush).
//
// FLAC_HOST_EMU compiles the same bodies as plain C++ (one lane at a time, wave maxima = the lane's own values) for host-side
// checking under a sanitizer; the library build never defines it.
#ifdef FLAC_HOST_EMU
#include <stdint.h>
#include <string.h>
#define FD static inline
#define FLAC_WMAX(v) (v)
#else
#include "common.h"
#define FD __device__ __forceinline__
FD int flac_wmax(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return __builtin_amdgcn_readfirstlane(v);
}
#define FLAC_WMAX(v) flac_wmax(v)
#endif

#define FLAC_TAB 16          // ints per file in the table
#define FLAC_REC 12          // ints per slot record
enum { FT_BEGIN, FT_END, FT_CH, FT_BPS, FT_MINBS, FT_MAXBS, FT_TOTAL, FT_ROW, FT_SLOT0, FT_SLOTS, FT_HASH0, FT_HASHN, FT_STAGE0 };
enum { FR_OFF, FR_FILE, FR_END, FR_ERR, FR_BS, FR_POS, FR_ASSIGN, FR_WASTED0, FR_WASTED1, FR_ACCEPT };
// status codes ([B][2]: code, then the byte offset for 1 and the frame index for the others)
enum { FS_OK, FS_OVERFLOW, FS_NO_FRAME, FS_RESERVED, FS_TRUNCATED, FS_CRC16, FS_POSITION, FS_TOO_MANY, FS_TOO_FEW };
enum { FE_RESERVED = 1, FE_TRUNCATED = 2, FE_CRC16 = 3 };
#define FLAC_RING 32
#define FLAC_LANES 64
// the ring's row pitch: 65 dwords, so that the flush below, which reads 16 rows x 2 columns per half wave, meets 32 different banks
// (bank = (row + lane) mod 32), while the sample loop's [row][lane] accesses stay on consecutive dwords
#define FLAC_RPITCH 65
// (make EXTRA=-DFLAC_STRIDED_STAGE builds the A/B partner of the flush: one dword per lane stored straight from the sample loop)
#define FLAC_REG_ORDER 8     // predictors of up to this many taps run from registers
#if defined(FLAC_HOST_EMU) || defined(FLAC_STRIDED_STAGE)
#define FLAC_FLUSH 0
#else
#define FLAC_FLUSH 1
#endif

struct FlacHeader {
    int ok, bs, assign, bps, hlen, variable;
    long long number;
};

// the frame header at byte `off` of the buffer (reads at most 16 bytes, none at or beyond `lim`); bps 0 = "as STREAMINFO says"
FD FlacHeader flac_header(const unsigned char* __restrict__ buf, long long off, long long lim) {
    FlacHeader h;
    h.ok = 0; h.bs = 0; h.assign = 0; h.bps = 0; h.hlen = 0; h.variable = 0; h.number = 0;
    unsigned char b[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) b[i] = 0;
    if (off < 0 || off + 2 > lim) return h;
    b[0] = buf[off]; b[1] = buf[off + 1];
    if (b[0] != 0xFF || (b[1] & 0xFE) != 0xF8) return h;
#pragma unroll
    for (int i = 2; i < 16; ++i) b[i] = off + i < lim ? buf[off + i] : 0;
    h.variable = b[1] & 1;
    const int bsc = b[2] >> 4, src = b[2] & 15, ssc = (b[3] >> 1) & 7;
    h.assign = b[3] >> 4;
    if (bsc == 0 || src == 15 || h.assign > 10 || ssc == 3 || ssc == 7 || (b[3] & 1)) return h;
    // the UTF-8-style number: 0xxxxxxx, or a lead byte of n ones and a zero followed by n - 1 bytes 10xxxxxx
    int n = 0;
    while (n < 8 && (b[4] & (0x80 >> n))) ++n;
    if (n == 1 || n == 8) return h;
    long long num = n ? (b[4] & (0x7F >> n)) : b[4];
    int p = 5;
#pragma unroll
    for (int k = 1; k < 7; ++k)
        if (k < n) {
            if ((b[4 + k] & 0xC0) != 0x80) return h;
            num = (num << 6) | (b[4 + k] & 0x3F);
            ++p;
        }
    if (!h.variable && n == 7) return h;                 // a frame number has 31 bits
    h.number = num;
    auto at = [&](int i) -> int {                        // b[i], i in 5 .. 15, without a runtime-indexed array
        int v = 0;
#pragma unroll
        for (int k = 5; k < 16; ++k) v = (k == i) ? b[k] : v;
        return v;
    };
    if (bsc == 1) h.bs = 192;
    else if (bsc <= 5) h.bs = 576 << (bsc - 2);
    else if (bsc == 6) { h.bs = at(p) + 1; p += 1; }
    else if (bsc == 7) { h.bs = ((at(p) << 8) | at(p + 1)) + 1; p += 2; }
    else h.bs = 256 << (bsc - 8);
    if (src == 12) p += 1;
    else if (src == 13 || src == 14) p += 2;
    h.bps = ssc == 0 ? 0 : ssc == 1 ? 8 : ssc == 2 ? 12 : ssc == 4 ? 16 : ssc == 5 ? 20 : 24;
    unsigned crc = 0;
#pragma unroll
    for (int k = 0; k < 15; ++k)
        if (k < p) {
            crc ^= b[k];
#pragma unroll
            for (int t = 0; t < 8; ++t) crc = (crc & 0x80) ? ((crc << 1) ^ 0x07) & 0xFF : (crc << 1) & 0xFF;
        }
    if (crc != (unsigned)at(p)) return h;
    h.hlen = p + 1;
    h.ok = 1;
    return h;
}

// header + STREAMINFO -> the candidate's sample position, or -1 when the two disagree
// (fixed blocking: frame number x the block size of the file's FIRST frame, which is STREAMINFO's minimum block size in every stream
// whose STREAMINFO tells the truth; the RFC's second example -- block sizes 4096 in STREAMINFO, frames of 16 and 3 -- does not)
FD long long flac_candidate(const FlacHeader& h, const int* __restrict__ ft, const FlacHeader& first) {
    if (!h.ok || !first.ok || h.variable != first.variable) return -1;
    const int want_ch = h.assign < 8 ? h.assign + 1 : 2;
    if (want_ch != ft[FT_CH] || (h.bps && h.bps != ft[FT_BPS]) || h.bs > ft[FT_MAXBS]) return -1;
    const long long pos = h.variable ? h.number : h.number * (long long)first.bs;
    if (pos >= (long long)ft[FT_TOTAL]) return -1;
    return pos;
}

FD unsigned flac_hash(unsigned off, unsigned n) { return ((off * 0x9E3779B1u) >> 8) & (n - 1); }

// ---- a. scan ------------------------------------------------------------------------------------------------------------------
FD void flac_scan_one(const unsigned char* __restrict__ buf, long long nbytes, const int* __restrict__ tab, int f, long long rel,
                      int* count, unsigned long long* hash, int* rec, int* status, int S, int H) {
    const int* ft = tab + f * FLAC_TAB;
    const long long begin = ft[FT_BEGIN], end = ft[FT_END] < nbytes ? ft[FT_END] : nbytes;
    const long long off = begin + rel;
    if (begin < 0 || off + 2 > end) return;
    if (buf[off] != 0xFF || (buf[off + 1] & 0xFE) != 0xF8) return;
    const FlacHeader h = flac_header(buf, off, end);
    if (!h.ok) return;
    const FlacHeader first = flac_header(buf, begin, end);
    if (flac_candidate(h, ft, first) < 0) return;
#ifdef FLAC_HOST_EMU
    const int n = count[f]++;
#else
    const int n = atomicAdd(&count[f], 1);
#endif
    const int slot = ft[FT_SLOT0] + n;
    if (n >= ft[FT_SLOTS] || slot < 0 || slot >= S) {
#ifdef FLAC_HOST_EMU
        if (status[2 * f] == 0) { status[2 * f] = FS_OVERFLOW; status[2 * f + 1] = (int)rel; }
#else
        if (atomicCAS(&status[2 * f], 0, FS_OVERFLOW) == 0) status[2 * f + 1] = (int)rel;
#endif
        return;
    }
    rec[slot * FLAC_REC + FR_OFF] = (int)off;
    rec[slot * FLAC_REC + FR_FILE] = f + 1;
    const unsigned hn = (unsigned)ft[FT_HASHN];
    const long long h0 = ft[FT_HASH0];
    if (hn == 0 || (hn & (hn - 1)) || h0 < 0 || h0 + hn > H) return;
    const unsigned long long key = ((unsigned long long)((unsigned)off + 1u) << 32) | (unsigned)slot;
    unsigned i = flac_hash((unsigned)off, hn);
    for (unsigned probe = 0; probe < hn; ++probe) {      // at most FT_SLOTS <= hn / 2 entries are ever taken
#ifdef FLAC_HOST_EMU
        if (hash[h0 + i] == 0) { hash[h0 + i] = key; return; }
#else
        if (atomicCAS(&hash[h0 + i], 0ull, key) == 0ull) return;
#endif
        i = (i + 1) & (hn - 1);
    }
}

FD int flac_lookup(const unsigned long long* __restrict__ hash, const int* __restrict__ ft, long long off, int H) {
    const unsigned hn = (unsigned)ft[FT_HASHN];
    const long long h0 = ft[FT_HASH0];
    if (hn == 0 || (hn & (hn - 1)) || h0 < 0 || h0 + hn > H) return -1;
    unsigned i = flac_hash((unsigned)off, hn);
    for (unsigned probe = 0; probe < hn; ++probe) {
        const unsigned long long e = hash[h0 + i];
        if (e == 0) return -1;
        if ((unsigned)(e >> 32) == (unsigned)off + 1u) return (int)(unsigned)e;
        i = (i + 1) & (hn - 1);
    }
    return -1;
}

// ---- b. decode ----------------------------------------------------------------------------------------------------------------
struct FlacBits {
    const unsigned* w;       // the buffer as dwords
    unsigned di, lim;        // index of the dword in `pre`; dwords at or beyond lim read as zero and are never loaded
    unsigned pre;            // the next dword, byte-swapped, loaded one refill ahead
    unsigned long long win;  // valid bits at the top, zeros below
    int nb;                  // valid bits in win
};
FD unsigned flac_ld(const FlacBits& r, unsigned i) { return i < r.lim ? __builtin_bswap32(r.w[i]) : 0u; }
FD void flac_refill(FlacBits& r) {
    if (r.nb <= 32) {
        r.win |= (unsigned long long)r.pre << (32 - r.nb);
        r.nb += 32;
        r.di += 1;
        r.pre = flac_ld(r, r.di);
    }
}
FD void flac_seek(FlacBits& r, long long byte) {
    r.di = (unsigned)(byte >> 2);
    r.win = 0; r.nb = 0;
    r.pre = flac_ld(r, r.di);
    flac_refill(r);
    flac_refill(r);
    const int skip = (int)(byte & 3) * 8;
    r.win <<= skip;
    r.nb -= skip;
}
FD long long flac_bitpos(const FlacBits& r) { return (long long)r.di * 32 - r.nb; }
FD unsigned flac_read(FlacBits& r, int n) {              // 0 <= n <= 32
    flac_refill(r);
    const unsigned v = (unsigned)((r.win >> 1) >> (63 - n));         // n == 0: shifted out entirely
    r.win <<= n;
    r.nb -= n;
    return v;
}
FD int flac_sext(unsigned v, int n) { return n ? (int)(v << (32 - n)) >> (32 - n) : 0; }
// zeros before the next one bit, which is consumed too; *bad is set when the run passes endbits
FD unsigned flac_unary(FlacBits& r, long long endbits, int* bad) {
    unsigned q = 0;
    flac_refill(r);
    while (r.win == 0) {
        q += (unsigned)r.nb;
        r.nb = 0;
        flac_refill(r);
        if (flac_bitpos(r) > endbits) { *bad = 1; return q; }
    }
    const int z = __builtin_clzll(r.win);
    q += (unsigned)z;
    r.win = (r.win << z) << 1;
    r.nb -= z + 1;
    return q;
}

FD int flac_fixed_coef(int order, int j) {
    const unsigned wd = order == 1 ? 0x00000001u : order == 2 ? 0x0000FF02u : order == 3 ? 0x0001FD03u : 0xFF04FA04u;
    return (j < order && j < 4) ? (int)(signed char)(wd >> (8 * j)) : 0;
}

// CRC-16 (0x8005, initial value 0, most significant bit first), four bytes a step: ct[k][x] = the CRC of byte x followed by k zero bytes
FD unsigned flac_crc16_byte(const unsigned short* __restrict__ ct, unsigned crc, unsigned b) {
    return ((crc << 8) & 0xFFFF) ^ ct[((crc >> 8) ^ b) & 0xFF];
}
FD unsigned flac_crc16(const unsigned char* __restrict__ buf, const unsigned short* __restrict__ ct, long long a, long long e) {
    unsigned crc = 0;
    while (a < e && (a & 3)) crc = flac_crc16_byte(ct, crc, buf[a++]);
    const unsigned* w = (const unsigned*)buf;
    for (; a + 4 <= e; a += 4) {
        const unsigned d = w[a >> 2];                    // little-endian: the first byte is the low one
        crc = ct[768 + (((crc >> 8) ^ d) & 0xFF)] ^ ct[512 + ((crc ^ (d >> 8)) & 0xFF)] ^ ct[256 + ((d >> 16) & 0xFF)] ^ ct[d >> 24];
    }
    while (a < e) crc = flac_crc16_byte(ct, crc, buf[a++]);
    return crc;
}
FD void flac_crc16_tables(unsigned short* ct, int t, int nt) {       // thread t of nt fills its share; the caller puts a barrier after it
    for (int x = t; x < 256; x += nt) {
        unsigned c = (unsigned)x << 8;
        for (int k = 0; k < 8; ++k) c = (c & 0x8000) ? ((c << 1) ^ 0x8005) & 0xFFFF : (c << 1) & 0xFFFF;
        ct[x] = (unsigned short)c;
    }
}
FD void flac_crc16_tables_more(unsigned short* ct, int t, int nt) {  // after the barrier: k zero bytes appended
    for (int x = t; x < 256; x += nt) {
        unsigned c = ct[x];
        for (int k = 1; k < 4; ++k) {
            c = ((c << 8) & 0xFFFF) ^ ct[c >> 8];
            ct[256 * k + x] = (unsigned short)c;
        }
    }
}

#if FLAC_FLUSH
// The last (up to) 16 samples of all 64 lanes, rows ii0 .. ii0 + 15 of the ring, to the staging areas: wave instruction t stores 16
// consecutive samples (64 bytes) of each of the four frames t, t + 16, t + 32, t + 48 -- whole 64-byte segments, where a store straight
// from the sample loop would touch 64 different lines with one dword each.  Called by the whole wave (the loop counter is uniform).
FD void flac_flush(const int* ring, const long long* s_base, const int* s_n, int* __restrict__ stage, long long stage_ints, int ii0, int lane) {
    __syncthreads();                                     // one wave per workgroup: orders the ring writes before these reads
    const int ii = ii0 + (lane & 15), g = lane >> 4;
#pragma unroll 4
    for (int t = 0; t < 16; ++t) {
        const int L = t + 16 * g;
        const long long a = s_base[L] + ii;
        if (ii < s_n[L] && a < stage_ints) stage[a] = ring[(ii & (FLAC_RING - 1)) * FLAC_RPITCH + L];
    }
}
#endif

// one candidate; ring [FLAC_RING][FLAC_RPITCH] and coef [FLAC_RING][FLAC_LANES] ints, this lane's column at `lane`.  Every lane of the wave calls this, with
// slot < 0 for a lane that has no candidate (the loop bounds are wave maxima)
FD void flac_decode_one(const unsigned char* __restrict__ buf, long long nbytes, const int* __restrict__ tab, int B, int* rec,
                        int* __restrict__ stage, long long stage_ints, int slot, int* ring, int* coef, const unsigned short* ct, int lane, long long* s_base, int* s_n) {
    int f = slot >= 0 ? rec[slot * FLAC_REC + FR_FILE] - 1 : -1;
    if (f >= B) f = -1;
    bool alive = f >= 0;
    const int* ft = tab + (alive ? f : 0) * FLAC_TAB;
    const long long end = alive ? (ft[FT_END] < nbytes ? ft[FT_END] : nbytes) : 0;
    const long long off = alive ? rec[slot * FLAC_REC + FR_OFF] : 0;
    const FlacHeader h = flac_header(buf, off, alive ? end : 0);
    long long pos = -1;
    const FlacHeader first = flac_header(buf, alive ? (long long)ft[FT_BEGIN] : 0, alive ? end : 0);
    if (alive) pos = flac_candidate(h, ft, first);
    alive = alive && pos >= 0;
    const int bs = alive ? h.bs : 0, nch = alive ? ft[FT_CH] : 0, bps = alive ? ft[FT_BPS] : 0;
    const long long endbits = end * 8;
    long long sbase = 0;
    if (alive) sbase = (long long)ft[FT_STAGE0] + (long long)(slot - ft[FT_SLOT0]) * nch * ft[FT_MAXBS];
    int err = 0;
    unsigned wasted_lo = 0, wasted_hi = 0;

    FlacBits r;
    r.w = (const unsigned*)buf;
    long long limb = (end + 15) / 16 * 16 + 16;          // the file's zero padding ends here
    if (limb > nbytes) limb = nbytes;
    r.lim = alive ? (unsigned)(limb >> 2) : 0u;
    flac_seek(r, off + h.hlen);

    const int max_ch = FLAC_WMAX(nch), max_bs = FLAC_WMAX(bs);
    for (int ch = 0; ch < max_ch; ++ch) {
        const bool act = alive && !err && ch < nch;
        // subframe header
        int width = bps + ((h.assign == 8 && ch == 1) || (h.assign == 9 && ch == 0) || (h.assign == 10 && ch == 1) ? 1 : 0);
        int order = 0, lpc = 0, fixed = 0, raw_only = 0, raw_w = 0, bad = 0, wasted = 0;
        if (act) {
            const unsigned hd = flac_read(r, 8);
            const int type = (hd >> 1) & 63;
            if (hd & 0x80) bad = 1;
            if (hd & 1) wasted = (int)flac_unary(r, endbits, &bad) + 1;
            if (wasted >= width) { bad = 1; wasted = 0; }
            width -= wasted;
            if (type == 0) { order = 1; fixed = 1; raw_only = 1; raw_w = 0; }            // constant
            else if (type == 1) { order = 0; raw_only = 1; raw_w = width; }              // verbatim
            else if (type >= 8 && type <= 12) { order = type - 8; fixed = 1; }
            else if (type >= 32) { order = (type & 31) + 1; lpc = 1; }
            else bad = 1;
            if (order > bs) bad = 1;
            if (bad) { err = FE_RESERVED; order = 0; }
        }
        bool on = act && !err;
        const int max_order = FLAC_WMAX(on ? order : 0);
        for (int i = 0; i < max_order; ++i)              // the warm-up samples
            if (on && i < order) ring[i * FLAC_RPITCH + lane] = flac_sext(flac_read(r, width), width);
        int prec = 0, shift = 0;
        if (on && lpc) {
            prec = (int)flac_read(r, 4) + 1;
            shift = flac_sext(flac_read(r, 5), 5);
            if (prec == 16 || shift < 0) { err = FE_RESERVED; on = false; shift = 0; }
        }
        for (int j = 0; j < max_order; ++j) {
            int c = 0;
            if (on && j < order) c = lpc ? flac_sext(flac_read(r, prec), prec) : flac_fixed_coef(order, j);
            coef[j * FLAC_LANES + lane] = c;
        }
        int method = 0, porder = 0;
        if (on && !raw_only) {
            method = (int)flac_read(r, 2);
            porder = (int)flac_read(r, 4);
            if (method > 1 || (porder && (bs & ((1 << porder) - 1))) || (bs >> porder) < order) { err = FE_RESERVED; on = false; }
        }
        int rem = raw_only ? bs - order : 0, part = 0, raw = raw_only, k = 0;
        const int pbits = method ? 5 : 4, plen = bs >> porder;
        const long long sch = sbase + (long long)ch * bs;
#if FLAC_FLUSH
        __syncthreads();                                 // the flushes of the channel before have read these
        s_base[lane] = sch;
        s_n[lane] = on ? bs : 0;
#endif
        // the residual of sample i (0 where the lane has none): the same code for every lane, a Rice code and a raw field differ in data only
        auto residual = [&](bool res) -> int {
            while (res && rem == 0 && on) {              // the next partition's header (the first partition may hold no residual)
                k = (int)flac_read(r, pbits);
                raw = k == (1 << pbits) - 1;
                if (raw) raw_w = (int)flac_read(r, 5);
                rem = plen - (part == 0 ? order : 0);
                if (++part > (1 << porder)) { err = FE_RESERVED; on = false; }
            }
            int v = 0;
            if (res && on) {
                unsigned q = 0;
                int over = 0;
                if (!raw) q = flac_unary(r, endbits, &over);
                const int nbits = raw ? raw_w : k;
                const unsigned low = flac_read(r, nbits);
                const unsigned u = (q << k) | low;
                v = raw ? flac_sext(low, raw_w) : (int)(u >> 1) ^ -(int)(u & 1);
                rem -= 1;
                if (over) { err = FE_TRUNCATED; on = false; }
            }
            return v;
        };
        auto emit = [&](int i, bool in) {
#if FLAC_FLUSH
            if ((i & 15) == 15 || i == max_bs - 1) flac_flush(ring, s_base, s_n, stage, stage_ints, i & ~15, lane);
#else
            if (in && sch + i < stage_ints) stage[sch + i] = ring[(i & (FLAC_RING - 1)) * FLAC_RPITCH + lane];
#endif
        };
        if (max_order <= FLAC_REG_ORDER) {
            // every predictor of the wave has at most 8 taps (libFLAC's presets up to -8 at 16 kHz; LibriSpeech): coefficients and
            // history in registers, statically indexed, so that the dependent chain of a sample holds no LDS round trip; the ring is
            // still written, for the flush
            int c[FLAC_REG_ORDER], hist[FLAC_REG_ORDER];
#pragma unroll
            for (int j = 0; j < FLAC_REG_ORDER; ++j) {
                c[j] = j < max_order ? coef[j * FLAC_LANES + lane] : 0;
                hist[j] = 0;
            }
            for (int i = 0; i < max_bs; ++i) {
                const bool in = on && i < bs;
                const bool res = in && i >= order;
                const int v = residual(res);
                long long acc = 0;
#pragma unroll
                for (int j = 0; j < FLAC_REG_ORDER; ++j) acc += (long long)c[j] * (long long)hist[j];
                int cur = (int)((unsigned)v + (unsigned)(acc >> shift));         // wraps on corrupt data, never on a valid stream
                if (i < max_order && !res) cur = ring[i * FLAC_RPITCH + lane];     // a warm-up sample (i is uniform: at most 8 reads)
#pragma unroll
                for (int j = FLAC_REG_ORDER - 1; j > 0; --j) hist[j] = hist[j - 1];
                hist[0] = cur;
                if (res) ring[(i & (FLAC_RING - 1)) * FLAC_RPITCH + lane] = cur;
                emit(i, in);
            }
        } else {
            for (int i = 0; i < max_bs; ++i) {
                const bool in = on && i < bs;
                const bool res = in && i >= order;
                const int v = residual(res);
                long long acc = 0;
                for (int j = 0; j < max_order; ++j)
                    acc += (long long)coef[j * FLAC_LANES + lane] * (long long)ring[((i - 1 - j) & (FLAC_RING - 1)) * FLAC_RPITCH + lane];
                const int s = (int)((unsigned)v + (unsigned)(acc >> shift));
                if (res) ring[(i & (FLAC_RING - 1)) * FLAC_RPITCH + lane] = s;
                emit(i, in);
            }
        }
        if (act && flac_bitpos(r) > endbits && !err) err = FE_TRUNCATED;
        if (ch < 4) wasted_lo |= (unsigned)wasted << (8 * ch);
        else wasted_hi |= (unsigned)wasted << (8 * (ch - 4));
    }
    // zero bits up to the byte boundary, then the CRC-16 of everything from the sync code on
    long long fin = (flac_bitpos(r) + 7) >> 3;
    if (alive && !err && fin + 2 > end) err = FE_TRUNCATED;
    if (alive && !err) {
        flac_seek(r, fin);
        const unsigned want = flac_read(r, 16);
        if (flac_crc16(buf, ct, off, fin) != want) err = FE_CRC16;
    }
    if (slot >= 0 && f >= 0) {
        int* rc = rec + slot * FLAC_REC;
        rc[FR_END] = (int)(fin + 2);
        rc[FR_ERR] = alive ? err : FE_RESERVED;
        rc[FR_BS] = bs;
        rc[FR_POS] = (int)pos;
        rc[FR_ASSIGN] = h.assign;
        rc[FR_WASTED0] = (int)wasted_lo;
        rc[FR_WASTED1] = (int)wasted_hi;
    }
}

// ---- c. chain -----------------------------------------------------------------------------------------------------------------
FD void flac_chain_one(const int* __restrict__ tab, int f, const unsigned long long* __restrict__ hash, int* rec, int* lengths,
                       int* status, long long nbytes, int S, int H) {
    const int* ft = tab + f * FLAC_TAB;
    const long long end = ft[FT_END] < nbytes ? ft[FT_END] : nbytes;
    long long cur = ft[FT_BEGIN];
    const int total = ft[FT_TOTAL];
    lengths[f] = total;
    if (status[2 * f]) return;                           // the scan ran out of slots
    long long expect = 0;
    int k = 0, code = 0;
    while (cur != end) {
        const int slot = flac_lookup(hash, ft, cur, H);
        if (slot < 0 || slot >= S || k >= ft[FT_SLOTS]) { code = FS_NO_FRAME; break; }
        int* rc = rec + slot * FLAC_REC;
        const int e = rc[FR_ERR];
        if (e) { code = e == FE_CRC16 ? FS_CRC16 : e == FE_TRUNCATED ? FS_TRUNCATED : FS_RESERVED; break; }
        if (rc[FR_POS] != expect) { code = FS_POSITION; break; }
        if (expect + rc[FR_BS] > total) { code = FS_TOO_MANY; break; }
        if (rc[FR_END] <= cur || rc[FR_END] > end) { code = FS_TRUNCATED; break; }
        rc[FR_ACCEPT] = 1;
        expect += rc[FR_BS];
        cur = rc[FR_END];
        ++k;
    }
    if (!code && expect != total) code = FS_TOO_FEW;
    status[2 * f] = code;
    status[2 * f + 1] = k;
}

// ---- d. commit ----------------------------------------------------------------------------------------------------------------
// sample i of an accepted slot: wave [B][Cw][Nmax] (Cw == 1: channel 0 only), pcm [B][Cp][Nmax] or NULL
FD void flac_commit_one(const int* __restrict__ tab, const int* __restrict__ rc, const int* __restrict__ stage, long long stage_ints,
                        int slot, int i, float* wave, int* pcm, int Cw, int Cp, int Nmax) {
    const int* ft = tab + (rc[FR_FILE] - 1) * FLAC_TAB;
    const int bs = rc[FR_BS], nch = ft[FT_CH], assign = rc[FR_ASSIGN];
    const long long t = (long long)rc[FR_POS] + i;
    if (i >= bs || t >= ft[FT_TOTAL] || t >= Nmax) return;
    const long long sbase = (long long)ft[FT_STAGE0] + (long long)(slot - ft[FT_SLOT0]) * nch * ft[FT_MAXBS];
    const float scale = __builtin_ldexpf(1.0f, 1 - ft[FT_BPS]);
    const long long row = ft[FT_ROW];
    auto get = [&](int ch) -> int {
        const long long a = sbase + (long long)ch * bs + i;
        const int w = ((ch < 4 ? rc[FR_WASTED0] : rc[FR_WASTED1]) >> (8 * (ch & 3))) & 31;
        return a < stage_ints ? (int)((unsigned)stage[a] << w) : 0;
    };
    auto put = [&](int ch, int v) {
        if (ch < Cw) wave[(row * Cw + ch) * Nmax + t] = (float)v * scale;
        if (pcm && ch < Cp) pcm[(row * Cp + ch) * Nmax + t] = v;
    };
    if (assign >= 8 && nch == 2) {
        const unsigned a = (unsigned)get(0), b = (unsigned)get(1);         // unsigned: defined whatever a CRC-valid frame holds
        int L, R;
        if (assign == 8) { L = (int)a; R = (int)(a - b); }
        else if (assign == 9) { L = (int)(a + b); R = (int)b; }
        else { const unsigned m = (a << 1) | (b & 1); L = (int)(m + b) >> 1; R = (int)(m - b) >> 1; }
        put(0, L);
        put(1, R);
    } else {
        for (int ch = 0; ch < nch; ++ch)
            if (ch < Cw || (pcm && ch < Cp)) put(ch, get(ch));
    }
}

// workspace: count [B] ints | hash [H] u64 | rec [S][FLAC_REC] ints (all three zeroed by the call) | staging [stage_ints] ints
struct FlacWs { long long count, hash, rec, stage, bytes, zeroed; };
static inline bool flac_ws_layout(int B, int S, int H, long long stage_ints, FlacWs* w) {
    if (B < 1 || S < 1 || H < 1 || stage_ints < 1 || stage_ints >= (1ll << 31) || S > (1 << 26) || H > (1 << 27)) return false;
    w->count = 0;
    w->hash = ((long long)B * 4 + 15) / 16 * 16;
    w->rec = w->hash + (long long)H * 8;
    w->zeroed = w->rec + (long long)S * FLAC_REC * 4;
    w->stage = (w->zeroed + 255) / 256 * 256;
    w->bytes = w->stage + stage_ints * 4;
    return true;
}

#ifndef FLAC_HOST_EMU
__global__ __launch_bounds__(256) void flac_scan_kernel(const unsigned char* __restrict__ buf, long long nbytes, const int* __restrict__ tab,
                                                        int* count, unsigned long long* hash, int* rec, int* status, int S, int H) {
    flac_scan_one(buf, nbytes, tab, blockIdx.y, (long long)blockIdx.x * 256 + threadIdx.x, count, hash, rec, status, S, H);
}

__global__ __launch_bounds__(64) void flac_decode_kernel(const unsigned char* __restrict__ buf, long long nbytes, const int* __restrict__ tab,
                                                         int B, int* rec, int* __restrict__ stage, long long stage_ints, int S) {
    __shared__ int ring[FLAC_RING * FLAC_RPITCH];
    __shared__ long long s_base[FLAC_LANES];
    __shared__ int s_n[FLAC_LANES];
    __shared__ int coef[FLAC_RING * FLAC_LANES];
    __shared__ unsigned short ct[4 * 256];
    const int lane = threadIdx.x;
    flac_crc16_tables(ct, lane, 64);
    __syncthreads();
    flac_crc16_tables_more(ct, lane, 64);
    __syncthreads();
    int slot = blockIdx.x * 64 + lane;
    if (slot >= S || rec[slot * FLAC_REC + FR_FILE] <= 0) slot = -1;
    if (FLAC_WMAX(slot) < 0) return;                     // wave-uniform: no candidate in these 64 slots
    flac_decode_one(buf, nbytes, tab, B, rec, stage, stage_ints, slot, ring, coef, ct, lane, s_base, s_n);
}

__global__ __launch_bounds__(64) void flac_chain_kernel(const int* __restrict__ tab, const unsigned long long* __restrict__ hash, int* rec,
                                                        int* lengths, int* status, long long nbytes, int B, int S, int H) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f < B) flac_chain_one(tab, f, hash, rec, lengths, status, nbytes, S, H);
}

__global__ __launch_bounds__(256) void flac_commit_kernel(const int* __restrict__ tab, const int* __restrict__ rec, const int* __restrict__ stage,
                                                          long long stage_ints, int B, float* wave, int* pcm, int Cw, int Cp, int Nmax) {
    const int slot = blockIdx.x;
    const int* rc = rec + slot * FLAC_REC;
    if (rc[FR_ACCEPT] != 1 || rc[FR_FILE] <= 0 || rc[FR_FILE] > B) return;
    const int bs = rc[FR_BS];
    for (int i = threadIdx.x; i < bs; i += 256) flac_commit_one(tab, rc, stage, stage_ints, slot, i, wave, pcm, Cw, Cp, Nmax);
}

extern "C" long long v100_flac_workspace_bytes(int B, int S, int H, long long stage_ints) {
    FlacWs w;
    return flac_ws_layout(B, S, H, stage_ints, &w) ? w.bytes : -1;
}

extern "C" int v100_flac_decode(const unsigned char* bytes, long long nbytes, const int* table, void* ws, float* wave, int* pcm,
                                int* lengths, int* status, int B, int S, int H, long long stage_ints, int max_file_bytes, int Cw, int Cp,
                                int Nmax, void* stream) {
    if (!bytes || !table || !ws || !wave || !lengths || !status) return V100_ERR_NULL;
    FlacWs w;
    if (!flac_ws_layout(B, S, H, stage_ints, &w) || B > 65535 || nbytes < 16 || nbytes >= (1ll << 31) || (nbytes & 15) || max_file_bytes < 1 ||
        max_file_bytes > nbytes || Cw < 1 || Cw > 8 || Cp < 1 || Cp > 8 || Nmax < 1)
        return V100_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    unsigned char* base = (unsigned char*)ws;
    int* count = (int*)(base + w.count);
    unsigned long long* hash = (unsigned long long*)(base + w.hash);
    int* rec = (int*)(base + w.rec);
    int* stage = (int*)(base + w.stage);
    if (hipMemsetAsync(base, 0, (size_t)w.zeroed, st) != hipSuccess) return V100_ERR_LAUNCH;
    if (hipMemsetAsync(status, 0, (size_t)B * 2 * sizeof(int), st) != hipSuccess) return V100_ERR_LAUNCH;
    V100_GGL(flac_scan_kernel, dim3(ceil_div(max_file_bytes, 256), B), dim3(256), 0, st, bytes, nbytes, table, count, hash, rec, status, S, H);
    V100_GGL(flac_decode_kernel, dim3(ceil_div(S, 64)), dim3(64), 0, st, bytes, nbytes, table, B, rec, stage, stage_ints, S);
    V100_GGL(flac_chain_kernel, dim3(ceil_div(B, 64)), dim3(64), 0, st, table, hash, rec, lengths, status, nbytes, B, S, H);
    V100_GGL(flac_commit_kernel, dim3(S), dim3(256), 0, st, table, rec, stage, stage_ints, B, wave, pcm, Cw, Cp, Nmax);
    return v100_launch_status();
}
#endif
