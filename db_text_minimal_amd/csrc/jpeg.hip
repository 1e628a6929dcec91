// Baseline JPEG decode for the device pipeline, in the place of the reference's cv2.imread(path)[:, :, ::-1]
// (data_loaders.py:78, utils.py:179): the serial, bit-granular entropy stage on the host, everything after it on the device.
//   host    dbn_jpeg_info            markers of one stream: size, components, sampling, restart interval, Exif orientation and
//                                    a support code; never reads past len
//           dbn_jpeg_coef_elems      int16 coefficients a batch needs (per image and in total)
//           dbn_jpeg_entropy_batch   Huffman-decodes N streams on up to min(N, 16, threads) threads into one int16 buffer —
//                                    per image and component the blocks of the MCU-padded grid in raster order, 64
//                                    coefficients each in NATURAL (de-zigzagged) order — plus an int64 descriptor per image,
//                                    one quantisation table per component and a status per image (a corrupt file fails alone)
//           dbn_jpeg_*_ex            the same three with a flags word (JF_MULTISCAN) and the Exif orientation of every header
//           dbn_jpeg_stream_plan     the host half of the device entropy stage (jpeg_dhuff.hip): the same headers, and the scans
//                                    cut at their markers into restart intervals, without reading a bit of the entropy data
//   device  dbn_jpeg_pixels          two kernels on one stream: jpeg_idct_kernel (dequantise, libjpeg's slow-integer 8 x 8
//                                    inverse DCT, + 128, clamp -> uint8 sample planes in a workspace) and jpeg_rgb_kernel
//                                    ("fancy" triangle chroma upsampling over the true downsampled size, YCbCr -> RGB or
//                                    grey x 3 -> packed uint8 [H][W][3] at the descriptor's byte offset).  Mixed sizes and
//                                    samplings run in one call: each workgroup looks its work up in a host-built table.
//           dbn_jpeg_pixels_ex       the same, and jpeg_rgb_oriented_kernel for the images the host lists as turned
// The arithmetic is libjpeg's (jidctint.c jpeg_idct_islow with CONST_BITS 13 / PASS1_BITS 2, jdsample.c h2v1 / h2v2
// fancy upsampling — plain replication when the downsampled width is 2 or less, as jinit_upsampler chooses — and jdcolor.c's
// 16-bit fixed-point tables), in int32; pinned bit for bit against Pillow / libjpeg-turbo through tests/jpeg_ref.py.  UNPINNED:
// IDCT results far outside the clamp range (corrupt data), where libjpeg indexes a masked table and this file clamps.
//
// Supported: SOF0 and 8-bit SOF1, 1 component or 3 (YCbCr), one interleaved scan, luma sampling 1x1 / 2x1 / 2x2 with 1x1
// chroma, DRI / RSTn, up to 4 Huffman and quantisation tables (8- or 16-bit entries), fill bytes and FF00 stuffing.  Every
// other kind is refused with its own status code (include/dbnet_hip.h).  The _ex entry points add two things, both off
// unless asked for: flag JF_MULTISCAN decodes SOF2 progressive Huffman streams and sequential streams of several scans on
// the host into the same coefficients (decode_scans), and dbn_jpeg_pixels_ex writes the images whose Exif orientation is
// 2 .. 8 turned, through a third, tiled kernel (jpeg_rgb_oriented_kernel).  The parser takes untrusted bytes: every read is
// checked against the end of the stream, and a decode writes only inside its image's slice of the coefficient buffer.
// The descriptor's fields, the zigzag order, the canonical code ranges and the thread pool are jpeg_common.h's.
#include <string.h>

#include "common.h"
#include "jpeg_common.h"
#include "jpeg_dhuff.h"

using namespace dbn_jpeg;

namespace {

enum {
    JS_OK = 0, JS_NOT_JPEG, JS_TRUNCATED, JS_PROGRESSIVE, JS_ARITHMETIC, JS_LOSSLESS, JS_PRECISION, JS_COMPONENTS, JS_SAMPLING,
    JS_MULTISCAN, JS_BAD_HEADER, JS_BAD_CODE, JS_COEF_RUN, JS_MARKER, JS_SCRIPT
};
enum { JF_MULTISCAN = 1 };  // flags of the _ex entry points: take progressive (SOF2) streams and sequential ones of several scans
constexpr int MAX_SCANS = 100;

constexpr int JP_INFO = 24;

// ---- host: markers ------------------------------------------------------------------------------------------------------
struct Huff {
    bool present = false;
    unsigned short fast[512];  // 9-bit prefix -> length << 8 | symbol, 0 when the code is longer
    int mincode[17], maxcode[17], first[17];
    unsigned char vals[256];
    int nvals = 0;
};

struct Header {
    int status = JS_OK;
    int width = 0, height = 0, ncomp = 0, sof = -1, precision = 0, ri = 0, orientation = 0, jfif = 0, adobe = -1;
    int cid[4] = {0, 0, 0, 0}, h[4] = {0, 0, 0, 0}, v[4] = {0, 0, 0, 0}, tq[4] = {0, 0, 0, 0};
    bool have_qt[4] = {false, false, false, false};
    unsigned short qt[4][64];  // natural order
    Huff dc[4], ac[4];
    int td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
    long scan_start = 0;
    bool multi = false;  // JF_MULTISCAN: SOF2, or a first scan that does not name every component; the scans are decode_scans'
    long sos_at = 0;     // multi: the length field of the first SOS segment
    unsigned short cqt[3][64];  // multi: per component the table in force at its first scan (decode_scans)
    // derived for a supported stream
    int hmax = 1, vmax = 1, mcux = 0, mcuy = 0, bw[3] = {0, 0, 0}, bh[3] = {0, 0, 0}, sh[3] = {1, 1, 1}, sv[3] = {1, 1, 1};
    long coef_elems() const {
        long n = 0;
        for (int c = 0; c < ncomp && c < 3; ++c) n += (long)bw[c] * bh[c] * 64;
        return n;
    }
};

bool build_huff(Huff& t, const unsigned char* counts, const unsigned char* vals, int nvals) {
    int k;
    if (!code_ranges(counts, t.mincode, t.maxcode, t.first, &k)) return false;
    memset(t.fast, 0, sizeof(t.fast));
    t.nvals = nvals;
    memcpy(t.vals, vals, nvals);
    for (int l = 1; l <= 9; ++l)
        for (int i = 0; i < counts[l - 1]; ++i) {
            const int c = (t.mincode[l] + i) << (9 - l);
            for (int j = 0; j < (1 << (9 - l)); ++j) t.fast[c + j] = (unsigned short)(l << 8 | vals[t.first[l] + i]);
        }
    t.present = true;
    return true;
}

int exif_orientation(const unsigned char* s, long n) {
    if (n < 14 || memcmp(s, "Exif\0\0", 6) != 0) return 0;
    const unsigned char* t = s + 6;
    const long tn = n - 6;
    bool le;
    if (t[0] == 'I' && t[1] == 'I') le = true;
    else if (t[0] == 'M' && t[1] == 'M') le = false;
    else return 0;
    auto u = [&](long o, int k, long* out) {
        if (o < 0 || o + k > tn) return false;
        long v = 0;
        for (int i = 0; i < k; ++i) v = v << 8 | t[le ? o + k - 1 - i : o + i];
        *out = v;
        return true;
    };
    long magic, ifd, cnt;
    if (!u(2, 2, &magic) || magic != 42 || !u(4, 4, &ifd) || !u(ifd, 2, &cnt)) return 0;
    for (long k = 0; k < cnt; ++k) {
        const long e = ifd + 2 + 12 * k;
        long tag, type, num, val;
        if (!u(e, 2, &tag) || !u(e + 8, 2, &val)) return 0;
        if (tag == 0x0112) {
            if (!u(e + 2, 2, &type) || !u(e + 4, 4, &num)) return 0;
            return (type == 3 && num == 1 && val >= 1 && val <= 8) ? (int)val : 0;
        }
    }
    return 0;
}

// DHT, DQT or DRI segment m with payload s[0 .. sn): its effect on the tables of hd -> a status
int table_segment(int m, const unsigned char* s, long sn, Header& hd) {
    if (m == 0xC4) {
        long q = 0;
        while (q < sn) {
            if (q + 17 > sn) return JS_BAD_HEADER;
            const int tc = s[q] >> 4, th = s[q] & 15;
            int tot = 0;
            for (int i = 0; i < 16; ++i) tot += s[q + 1 + i];
            if (tc > 1 || th > 3 || tot > 256 || q + 17 + tot > sn) return JS_BAD_HEADER;
            if (!build_huff(tc == 0 ? hd.dc[th] : hd.ac[th], s + q + 1, s + q + 17, tot)) return JS_BAD_HEADER;
            q += 17 + tot;
        }
    } else if (m == 0xDB) {
        long q = 0;
        while (q < sn) {
            const int pq = s[q] >> 4, tq = s[q] & 15;
            const int need = pq ? 128 : 64;
            if (pq > 1 || tq > 3 || q + 1 + need > sn) return JS_BAD_HEADER;
            for (int k = 0; k < 64; ++k)
                hd.qt[tq][kZigzag[k]] = pq ? (unsigned short)(s[q + 1 + 2 * k] << 8 | s[q + 2 + 2 * k]) : s[q + 1 + k];
            hd.have_qt[tq] = true;
            q += 1 + need;
        }
    } else if (m == 0xDD) {
        if (sn != 2) return JS_BAD_HEADER;
        hd.ri = s[0] << 8 | s[1];
    }
    return JS_OK;
}

// parses up to and including the first SOS header; hd.status tells whether the scan (hd.multi: the scans) can be decoded
void parse_header(const unsigned char* d, long n, Header& hd, int flags = 0) {
    auto fail = [&](int s) { hd.status = s; };
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return fail(JS_NOT_JPEG);
    long p = 2;
    for (;;) {
        if (p >= n) return fail(JS_TRUNCATED);
        if (d[p] != 0xFF) return fail(JS_BAD_HEADER);
        while (p < n && d[p] == 0xFF) ++p;
        if (p >= n) return fail(JS_TRUNCATED);
        const int m = d[p++];
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
        if (m == 0xD9) return fail(JS_BAD_HEADER);
        if (p + 2 > n) return fail(JS_TRUNCATED);
        const long L = d[p] << 8 | d[p + 1];
        if (L < 2) return fail(JS_BAD_HEADER);
        if (p + L > n) return fail(JS_TRUNCATED);
        const unsigned char* s = d + p + 2;
        const long sn = L - 2;
        p += L;
        if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
            if (hd.sof >= 0) return fail(JS_BAD_HEADER);
            if (m == 0xC2 && !(flags & JF_MULTISCAN)) return fail(JS_PROGRESSIVE);
            if (m == 0xC9 || m == 0xCA || m == 0xCB || m == 0xCD || m == 0xCE || m == 0xCF) return fail(JS_ARITHMETIC);
            if (m == 0xC3 || m == 0xC5 || m == 0xC6 || m == 0xC7) return fail(JS_LOSSLESS);
            if (sn < 6) return fail(JS_BAD_HEADER);
            hd.precision = s[0];
            if (s[0] != 8) return fail(JS_PRECISION);
            hd.sof = m - 0xC0;
            hd.height = s[1] << 8 | s[2];
            hd.width = s[3] << 8 | s[4];
            hd.ncomp = s[5];
            if (hd.height == 0 || hd.width == 0 || hd.ncomp == 0 || sn != 6 + 3 * hd.ncomp) return fail(JS_BAD_HEADER);
            for (int c = 0; c < hd.ncomp && c < 4; ++c) {
                hd.cid[c] = s[6 + 3 * c];
                hd.h[c] = s[7 + 3 * c] >> 4;
                hd.v[c] = s[7 + 3 * c] & 15;
                hd.tq[c] = s[8 + 3 * c];
            }
        } else if (m == 0xC8) {
            return fail(JS_BAD_HEADER);
        } else if (m == 0xCC) {
            return fail(JS_ARITHMETIC);
        } else if (m == 0xC4 || m == 0xDB || m == 0xDD) {
            const int st = table_segment(m, s, sn, hd);
            if (st != JS_OK) return fail(st);
        } else if (m == 0xE0) {
            if (sn >= 5 && memcmp(s, "JFIF\0", 5) == 0) hd.jfif = 1;
        } else if (m == 0xE1) {
            if (hd.orientation == 0) hd.orientation = exif_orientation(s, sn);
        } else if (m == 0xEE) {
            if (sn >= 12 && memcmp(s, "Adobe", 5) == 0) hd.adobe = s[11];
        } else if (m == 0xDA) {
            if (hd.sof < 0 || sn < 1) return fail(JS_BAD_HEADER);
            if ((hd.ncomp != 1 && hd.ncomp != 3) || (hd.ncomp == 3 && hd.adobe == 0)) return fail(JS_COMPONENTS);
            if (hd.ncomp == 3) {
                const bool luma = (hd.h[0] == 1 && hd.v[0] == 1) || (hd.h[0] == 2 && hd.v[0] == 1) || (hd.h[0] == 2 && hd.v[0] == 2);
                if (!luma || hd.h[1] != 1 || hd.v[1] != 1 || hd.h[2] != 1 || hd.v[2] != 1) return fail(JS_SAMPLING);
            }
            const int ns = s[0];
            if (ns != hd.ncomp || hd.sof == 2) {
                if (!(flags & JF_MULTISCAN)) return fail(JS_MULTISCAN);
                for (int c = 0; c < hd.ncomp; ++c)
                    if (hd.tq[c] > 3) return fail(JS_BAD_HEADER);
                hd.multi = true;
                hd.sos_at = p - L;
                break;
            }
            if (sn != 4 + 2 * ns) return fail(JS_BAD_HEADER);
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != hd.cid[c]) return fail(JS_BAD_HEADER);
                hd.td[c] = s[2 + 2 * c] >> 4;
                hd.ta[c] = s[2 + 2 * c] & 15;
                if (hd.td[c] > 3 || hd.ta[c] > 3 || hd.tq[c] > 3) return fail(JS_BAD_HEADER);
                if (!hd.dc[hd.td[c]].present || !hd.ac[hd.ta[c]].present || !hd.have_qt[hd.tq[c]]) return fail(JS_BAD_HEADER);
            }
            hd.scan_start = p;
            break;
        }
    }
    if (hd.ncomp == 3) {
        hd.hmax = hd.h[0];
        hd.vmax = hd.v[0];
        for (int c = 0; c < 3; ++c) hd.sh[c] = hd.h[c], hd.sv[c] = hd.v[c];
    }
    hd.mcux = (hd.width + 8 * hd.hmax - 1) / (8 * hd.hmax);
    hd.mcuy = (hd.height + 8 * hd.vmax - 1) / (8 * hd.vmax);
    for (int c = 0; c < hd.ncomp; ++c) hd.bw[c] = hd.mcux * hd.sh[c], hd.bh[c] = hd.mcuy * hd.sv[c];
}

// ---- host: the entropy-coded segment ------------------------------------------------------------------------------------
// The stream as bits: FF00 unstuffed, fill bytes skipped, stopped at a marker or the end of the data, past which zeros are
// supplied and counted (`fake`), so that a decode which runs into them is found out (overrun) instead of reading further.
struct Bits {
    const unsigned char* d;
    long p, n;
    unsigned long long acc = 0;
    int bits = 0;
    int marker = 0;  // 0 none yet, -1 end of data, else the marker's code
    long fake = 0;

    inline unsigned byte() {
        if (marker != 0) { fake += 8; return 0; }
        if (p >= n) { marker = -1; fake += 8; return 0; }
        const unsigned b = d[p++];
        if (b != 0xFF) return b;
        for (;;) {
            if (p >= n) { marker = -1; break; }
            const unsigned m = d[p++];
            if (m == 0) return 0xFF;
            if (m != 0xFF) { marker = (int)m; break; }
        }
        fake += 8;
        return 0;
    }
    inline void fill() {  // at least 33 bits afterwards: one code (16) and one value (16) without refilling
        while (bits <= 32) {
            acc = acc << 8 | byte();
            bits += 8;
        }
    }
    inline unsigned peek(int k) const { return (unsigned)(acc >> (bits - k)) & ((1u << k) - 1); }
    inline bool overrun() const { return marker != 0 && bits < fake; }
    // the padding bits dropped, the next thing must be a marker: its code, or a negative status
    int end_interval() {
        if (overrun()) return marker == -1 ? -JS_TRUNCATED : -JS_MARKER;
        const long real = marker != 0 ? bits - fake : bits;
        if (real >= 8) return -JS_MARKER;
        if (marker == 0) {
            if (p >= n) return -JS_TRUNCATED;
            if (d[p] != 0xFF) return -JS_MARKER;
            while (p < n && d[p] == 0xFF) ++p;
            if (p >= n) return -JS_TRUNCATED;
            const int m = d[p++];
            if (m == 0) return -JS_MARKER;
            marker = m;
        }
        if (marker == -1) return -JS_TRUNCATED;
        const int m = marker;
        acc = 0, bits = 0, fake = 0, marker = 0;
        return m;
    }
};

// one Huffman symbol (after fill()): -1 for a code that is in no table
inline int huff_symbol(Bits& b, const Huff& t) {
    const unsigned f = t.fast[b.peek(9)];
    if (f) {
        b.bits -= f >> 8;
        return f & 255;
    }
    for (int l = 10; l <= 16; ++l) {
        const int code = (int)b.peek(l);
        if (t.maxcode[l] >= 0 && code >= t.mincode[l] && code <= t.maxcode[l]) {
            const int i = t.first[l] + code - t.mincode[l];
            if (i >= t.nvals) return -1;
            b.bits -= l;
            return t.vals[i];
        }
    }
    return -1;
}

inline int receive_extend(Bits& b, int s) {
    if (s == 0) return 0;
    const int v = (int)b.peek(s);
    b.bits -= s;
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// one block of a sequential scan (T.81 F.2.2) into k64 (zeroed), natural order; pred: the component's DC predictor
inline int sequential_block(Bits& b, const Huff& dc, const Huff& ac, int& pred, short* k64) {
    b.fill();
    int s = huff_symbol(b, dc);
    if (s < 0 || s > 11) return JS_BAD_CODE;
    pred = (short)(pred + receive_extend(b, s));
    k64[0] = (short)pred;
    int k = 1;
    while (k < 64) {
        b.fill();
        const int rs = huff_symbol(b, ac);
        if (rs < 0) return JS_BAD_CODE;
        const int r = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (r != 15) break;
            k += 16;
            if (k > 64) return JS_COEF_RUN;
            continue;
        }
        k += r;
        if (k > 63) return JS_COEF_RUN;
        k64[kZigzag[k]] = (short)receive_extend(b, s);
        ++k;
    }
    return JS_OK;
}

// decodes the scan of a parsed, supported stream into coef[0 .. hd.coef_elems()) (zeroed here): a status
int decode_scan(const unsigned char* d, long n, const Header& hd, short* coef) {
    const long total = hd.coef_elems();
    memset(coef, 0, (size_t)total * sizeof(short));
    long comp_off[3] = {0, 0, 0};
    for (int c = 1; c < hd.ncomp; ++c) comp_off[c] = comp_off[c - 1] + (long)hd.bw[c - 1] * hd.bh[c - 1] * 64;
    Bits b{d, hd.scan_start, n};
    int pred[3] = {0, 0, 0};
    const long mcus = (long)hd.mcux * hd.mcuy;
    long to_restart = hd.ri;
    int next_rst = 0;
    for (long mcu = 0; mcu < mcus; ++mcu) {
        if (hd.ri && mcu && to_restart == 0) {
            const int m = b.end_interval();
            if (m < 0) return -m;
            if (m != 0xD0 + next_rst) return JS_MARKER;
            next_rst = (next_rst + 1) & 7;
            pred[0] = pred[1] = pred[2] = 0;
            to_restart = hd.ri;
        }
        --to_restart;
        const long my = mcu / hd.mcux, mx = mcu - my * hd.mcux;
        for (int c = 0; c < hd.ncomp; ++c) {
            const Huff& dc = hd.dc[hd.td[c]];
            const Huff& ac = hd.ac[hd.ta[c]];
            for (int v = 0; v < hd.sv[c]; ++v)
                for (int u = 0; u < hd.sh[c]; ++u) {
                    const long blk = (my * hd.sv[c] + v) * hd.bw[c] + mx * hd.sh[c] + u;
                    const long o = comp_off[c] + blk * 64;
                    if (o < 0 || o + 64 > total) return JS_BAD_HEADER;  // cannot happen for a grid derived above
                    const int st = sequential_block(b, dc, ac, pred[c], coef + o);
                    if (st != JS_OK) return st;
                }
        }
        if (b.overrun()) return b.marker == -1 ? JS_TRUNCATED : JS_MARKER;
    }
    const int m = b.end_interval();
    if (m < 0) return -m;
    if (m >= 0xD0 && m <= 0xD7) return JS_MARKER;
    return JS_OK;
}

// ---- host: streams of more than one scan (JF_MULTISCAN) ----------------------------------------------------------------------
// Progressive Huffman streams (T.81 Annex G) and sequential streams whose components come in several scans.  The walker goes
// on from the first SOS through every scan to EOI; DHT, DQT and DRI between scans hold for the scans that follow, and a
// component's quantisation table is the one in force at its first scan.  A scan of one component walks that component's real
// block grid (its restart interval counts blocks), a scan of several walks MCUs over the padded grid; blocks no scan sends
// stay zero.  sent[c][k]: the Al coefficient k of component c was last sent with, -1 never; the script is complete when all
// are 0 at EOI.  Stricter than libjpeg, which only warns: a band sent first twice, a refinement that does not continue
// the band's last Al, an AC scan before the component's DC, a sequential scan with spectral selection, a component in two
// sequential scans and a refinement symbol of size > 1 are all malformed here.
inline unsigned get_bit(Bits& b) {
    if (b.bits == 0) b.fill();
    --b.bits;
    return (unsigned)(b.acc >> b.bits) & 1;
}

struct ScanSpec {
    int ns, ci[3], td[3], ta[3], Ss, Se, Ah, Al;
};

// the correction bit of a coefficient that is already non-zero (G.1.2.3)
inline void refine_nonzero(Bits& b, short& v, int p1) {
    if (get_bit(b) && (v & p1) == 0) v = (short)(v >= 0 ? v + p1 : v - p1);
}

// one block of a progressive scan; eob: the end-of-band run still to go
inline int progressive_block(Bits& b, const ScanSpec& sc, const Huff* dc, const Huff* ac, int& pred, int& eob, short* k64) {
    const int Al = sc.Al, p1 = 1 << Al;
    if (sc.Ss == 0) {
        if (sc.Ah) {  // DC refinement: one bit
            if (get_bit(b)) k64[0] = (short)(k64[0] | p1);
            return JS_OK;
        }
        b.fill();
        const int s = huff_symbol(b, *dc);
        if (s < 0 || s > 11) return JS_BAD_CODE;
        pred = (short)(pred + receive_extend(b, s));
        k64[0] = (short)((unsigned)pred << Al);
        return JS_OK;
    }
    int k = sc.Ss;
    if (sc.Ah == 0) {  // AC first
        if (eob > 0) {
            --eob;
            return JS_OK;
        }
        while (k <= sc.Se) {
            b.fill();
            const int rs = huff_symbol(b, *ac);
            if (rs < 0) return JS_BAD_CODE;
            const int r = rs >> 4, s = rs & 15;
            if (s == 0) {
                if (r != 15) {
                    eob = (1 << r) - 1;
                    if (r) {
                        eob += (int)b.peek(r);
                        b.bits -= r;
                    }
                    break;
                }
                k += 16;
                if (k > sc.Se + 1) return JS_COEF_RUN;
                continue;
            }
            k += r;
            if (k > sc.Se) return JS_COEF_RUN;
            k64[kZigzag[k]] = (short)((unsigned)receive_extend(b, s) << Al);
            ++k;
        }
        return JS_OK;
    }
    if (eob == 0) {  // AC refinement
        while (k <= sc.Se) {
            b.fill();
            const int rs = huff_symbol(b, *ac);
            if (rs < 0) return JS_BAD_CODE;
            int r = rs >> 4;
            const int s = rs & 15;
            int val = 0;
            if (s) {
                if (s != 1) return JS_BAD_CODE;
                val = get_bit(b) ? p1 : -p1;
            } else if (r != 15) {
                eob = 1 << r;
                if (r) {
                    b.fill();
                    eob += (int)b.peek(r);
                    b.bits -= r;
                }
                break;
            }
            for (; k <= sc.Se; ++k) {  // over the non-zero coefficients and r zero ones
                short& v = k64[kZigzag[k]];
                if (v != 0) refine_nonzero(b, v, p1);
                else if (--r < 0) break;
            }
            if (k > sc.Se) return JS_COEF_RUN;  // the band ended before the run did
            if (s) k64[kZigzag[k]] = (short)val;
            ++k;
        }
    }
    if (eob > 0) {
        for (; k <= sc.Se; ++k) {
            short& v = k64[kZigzag[k]];
            if (v != 0) refine_nonzero(b, v, p1);
        }
        --eob;
    }
    return JS_OK;
}

// the entropy data of one scan, from byte p; *next: the marker that ends it, *pend: the byte behind that marker
int decode_one_scan(const unsigned char* d, long n, long p, const Header& hd, const ScanSpec& sc, short* coef, const long* comp_off, long total,
                    int* next, long* pend) {
    Bits b{d, p, n};
    int pred[3] = {0, 0, 0}, eob = 0;
    const bool prog = hd.sof == 2;
    long ux, units;  // units per row and in all: blocks of the component's real grid, or MCUs
    int c0 = sc.ci[0];
    if (sc.ns == 1) {
        const long cw = ((long)hd.width * hd.sh[c0] + hd.hmax - 1) / hd.hmax, ch = ((long)hd.height * hd.sv[c0] + hd.vmax - 1) / hd.vmax;
        ux = (cw + 7) / 8;
        units = ux * ((ch + 7) / 8);
    } else {
        ux = hd.mcux;
        units = (long)hd.mcux * hd.mcuy;
    }
    long to_restart = hd.ri;
    int next_rst = 0;
    for (long u = 0; u < units; ++u) {
        if (hd.ri && u && to_restart == 0) {
            const int m = b.end_interval();
            if (m < 0) return -m;
            if (m != 0xD0 + next_rst) return JS_MARKER;
            next_rst = (next_rst + 1) & 7;
            pred[0] = pred[1] = pred[2] = 0;
            eob = 0;
            to_restart = hd.ri;
        }
        --to_restart;
        const long uy = u / ux, uxx = u - uy * ux;
        for (int i = 0; i < sc.ns; ++i) {
            const int c = sc.ci[i];
            const int nv = sc.ns == 1 ? 1 : hd.sv[c], nh = sc.ns == 1 ? 1 : hd.sh[c];
            const Huff* dc = &hd.dc[sc.td[i]];
            const Huff* ac = &hd.ac[sc.ta[i]];
            for (int v = 0; v < nv; ++v)
                for (int h = 0; h < nh; ++h) {
                    const long blk = (uy * nv + v) * hd.bw[c] + uxx * nh + h;
                    const long o = comp_off[c] + blk * 64;
                    if (blk < 0 || blk >= (long)hd.bw[c] * hd.bh[c] || o + 64 > total) return JS_BAD_HEADER;  // cannot happen for these grids
                    const int st = prog ? progressive_block(b, sc, dc, ac, pred[c], eob, coef + o) : sequential_block(b, *dc, *ac, pred[c], coef + o);
                    if (st != JS_OK) return st;
                }
        }
        if (b.overrun()) return b.marker == -1 ? JS_TRUNCATED : JS_MARKER;
    }
    const int m = b.end_interval();
    if (m < 0) return -m;
    if (m >= 0xD0 && m <= 0xD7) return JS_MARKER;
    *next = m, *pend = b.p;
    return JS_OK;
}

// every scan of a parsed hd.multi stream into coef[0 .. hd.coef_elems()) (zeroed here), the tables into hd.cqt: a status.
// nscans (may be null): the scans decoded.  hd's Huffman, quantisation tables and restart interval follow the stream.
int decode_scans(const unsigned char* d, long n, Header& hd, short* coef, int* nscans) {
    const long total = hd.coef_elems();
    memset(coef, 0, (size_t)total * sizeof(short));
    memset(hd.cqt, 0, sizeof(hd.cqt));
    long comp_off[3] = {0, 0, 0};
    for (int c = 1; c < hd.ncomp; ++c) comp_off[c] = comp_off[c - 1] + (long)hd.bw[c - 1] * hd.bh[c - 1] * 64;
    signed char sent[3][64];
    memset(sent, -1, sizeof(sent));
    bool begun[3] = {false, false, false};
    long p = hd.sos_at;
    int m = 0xDA, scans = 0;
    for (;;) {
        if (m == 0) {  // the next marker, as parse_header reads it
            if (p >= n) return JS_TRUNCATED;
            if (d[p] != 0xFF) return JS_BAD_HEADER;
            while (p < n && d[p] == 0xFF) ++p;
            if (p >= n) return JS_TRUNCATED;
            m = d[p++];
        }
        if (m == 0xD9) break;
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) {
            m = 0;
            continue;
        }
        if (p + 2 > n) return JS_TRUNCATED;
        const long L = d[p] << 8 | d[p + 1];
        if (L < 2) return JS_BAD_HEADER;
        if (p + L > n) return JS_TRUNCATED;
        const unsigned char* s = d + p + 2;
        const long sn = L - 2;
        p += L;
        const int seg = m;
        m = 0;
        if (seg == 0xCC) return JS_ARITHMETIC;
        if (seg >= 0xC0 && seg <= 0xCF && seg != 0xC4) return JS_BAD_HEADER;  // a second frame header
        if (seg != 0xDA) {
            const int st = table_segment(seg, s, sn, hd);
            if (st != JS_OK) return st;
            continue;
        }
        if (++scans > MAX_SCANS) return JS_SCRIPT;
        ScanSpec sc;
        if (sn < 1) return JS_BAD_HEADER;
        sc.ns = s[0];
        if (sc.ns < 1 || sc.ns > hd.ncomp || sn != 4 + 2 * sc.ns) return JS_BAD_HEADER;
        for (int i = 0; i < sc.ns; ++i) {
            int c = 0;
            while (c < hd.ncomp && hd.cid[c] != s[1 + 2 * i]) ++c;
            if (c == hd.ncomp || (i && c <= sc.ci[i - 1])) return JS_BAD_HEADER;  // components in the frame's order
            sc.ci[i] = c, sc.td[i] = s[2 + 2 * i] >> 4, sc.ta[i] = s[2 + 2 * i] & 15;
            if (sc.td[i] > 3 || sc.ta[i] > 3) return JS_BAD_HEADER;
        }
        sc.Ss = s[1 + 2 * sc.ns], sc.Se = s[2 + 2 * sc.ns], sc.Ah = s[3 + 2 * sc.ns] >> 4, sc.Al = s[3 + 2 * sc.ns] & 15;
        const bool prog = hd.sof == 2;
        if (prog) {
            if (sc.Ss == 0 ? sc.Se != 0 : (sc.ns > 1 || sc.Se < sc.Ss || sc.Se > 63)) return JS_BAD_HEADER;
            if (sc.Al > 13 || (sc.Ah != 0 && sc.Ah != sc.Al + 1)) return JS_BAD_HEADER;
        } else if (sc.Ss != 0 || sc.Se != 63 || sc.Ah != 0 || sc.Al != 0) {
            return JS_BAD_HEADER;
        }
        for (int i = 0; i < sc.ns; ++i) {
            const int c = sc.ci[i];
            if (prog && sc.Ss > 0 && sent[c][0] < 0) return JS_BAD_HEADER;  // AC before the component's first DC scan
            for (int k = sc.Ss; k <= sc.Se; ++k) {
                if (sent[c][k] != (sc.Ah ? sc.Ah : -1)) return JS_BAD_HEADER;  // sent twice, or not the refinement that is due
                sent[c][k] = (signed char)sc.Al;
            }
            const bool need_dc = !prog || (sc.Ss == 0 && sc.Ah == 0), need_ac = !prog || sc.Ss > 0;
            if ((need_dc && !hd.dc[sc.td[i]].present) || (need_ac && !hd.ac[sc.ta[i]].present)) return JS_BAD_HEADER;
            if (!begun[c]) {
                if (!hd.have_qt[hd.tq[c]]) return JS_BAD_HEADER;
                memcpy(hd.cqt[c], hd.qt[hd.tq[c]], sizeof(hd.cqt[c]));
                begun[c] = true;
            }
        }
        const int st = decode_one_scan(d, n, p, hd, sc, coef, comp_off, total, &m, &p);
        if (st != JS_OK) return st;
    }
    if (nscans) *nscans = scans;
    for (int c = 0; c < hd.ncomp; ++c)
        for (int k = 0; k < 64; ++k)
            if (sent[c][k] != 0) return JS_SCRIPT;
    return JS_OK;
}

// the scans of a stream from its first SOS on, by the markers alone: segments are stepped over by their lengths, entropy data
// up to the next FF that is followed by neither 00, FF nor RSTn (dbn_jpeg_info_ex)
int count_scans(const unsigned char* d, long n, long sos_at) {
    int scans = 0, m = 0xDA;
    long p = sos_at;
    for (;;) {
        if (m == 0) {
            if (p >= n || d[p] != 0xFF) return scans;
            while (p < n && d[p] == 0xFF) ++p;
            if (p >= n) return scans;
            m = d[p++];
        }
        if (m == 0xD9) return scans;
        const bool alone = m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7);
        const bool sos = m == 0xDA;
        m = 0;
        if (alone) continue;
        if (p + 2 > n) return scans;
        const long L = d[p] << 8 | d[p + 1];
        if (L < 2 || p + L > n) return scans;
        p += L;
        if (!sos) continue;
        ++scans;
        while (m == 0) {
            const unsigned char* f = p < n ? (const unsigned char*)memchr(d + p, 0xFF, (size_t)(n - p)) : nullptr;
            if (!f || f - d + 1 >= n) return scans;
            p = f - d + 1;
            const int x = d[p];
            if (x == 0xFF) continue;
            ++p;
            if (x != 0 && !(x >= 0xD0 && x <= 0xD7)) m = x;
        }
    }
}

// ---- host: descriptors ----------------------------------------------------------------------------------------------------
// image n's descriptor and quantisation tables; co / oo: where its coefficients and its pixels start, moved on behind
// them.  false: the coefficients do not fit into coef_elems.
bool describe(const Header& hd, int n, long coef_elems, long& co, long& oo, long long* d, unsigned short* q) {
    for (int i = 0; i < JP_DESC; ++i) d[i] = 0;
    memset(q, 0, 192 * sizeof(unsigned short));
    d[D_STATUS] = hd.status;
    d[D_COEF] = co, d[D_OUT] = oo, d[D_QT] = (long)n * 192;
    if (hd.status != JS_OK) return true;
    if (co + hd.coef_elems() > coef_elems) return false;
    d[D_W] = hd.width, d[D_H] = hd.height, d[D_NC] = hd.ncomp;
    for (int c = 0; c < hd.ncomp; ++c) {
        d[D_COMP + 4 * c] = hd.bw[c], d[D_COMP + 4 * c + 1] = hd.bh[c], d[D_COMP + 4 * c + 2] = hd.sh[c], d[D_COMP + 4 * c + 3] = hd.sv[c];
        if (!hd.multi) memcpy(q + 64 * c, hd.qt[hd.tq[c]], 64 * sizeof(unsigned short));  // multi: after its scans, from hd.cqt
    }
    d[D_HMAX] = hd.hmax, d[D_VMAX] = hd.vmax, d[D_MCUX] = hd.mcux, d[D_MCUY] = hd.mcuy, d[D_RI] = hd.ri;
    co += hd.coef_elems();
    oo += (long)hd.width * hd.height * 3;
    return true;
}

// ---- host: the plan of the device entropy stage (jpeg_dhuff.hip) ---------------------------------------------------------------
// The restart intervals of a parsed, supported stream, found from the FF xx pairs of its scan alone: no bit of the entropy
// data is looked at.  rows: DH_SEG int64 per interval (offsets relative to `d`), or nullptr to count.  -> the number of
// intervals, or -1 when the markers are not the ones the header calls for (a marker missing, one too many, a wrong RSTn,
// fill bytes, the end of the data): such a scan is the host decoder's.
long scan_segments(const unsigned char* d, long n, const Header& hd, std::vector<long long>* rows) {
    using namespace dbn_dhuff;
    const long mcus = (long)hd.mcux * hd.mcuy;
    const long want = hd.ri ? (mcus + hd.ri - 1) / hd.ri : 1;
    long p = hd.scan_start, first = p, k = 0;
    for (;;) {
        const unsigned char* f = p < n ? (const unsigned char*)memchr(d + p, 0xFF, (size_t)(n - p)) : nullptr;
        if (!f) return -1;
        const long q = f - d;
        if (q + 1 >= n) return -1;
        const int m = d[q + 1];
        if (m == 0) {
            p = q + 2;
            continue;
        }
        if (m == 0xFF) return -1;
        if ((q - first) * 8 > 0xFFFFFFF0L) return -1;
        const bool rst = m >= 0xD0 && m <= 0xD7;
        if (rst ? (k >= want - 1 || m != 0xD0 + (int)(k & 7)) : k != want - 1) return -1;
        if (rows) {
            const long long row[DH_SEG] = {0, first, q, hd.ri ? k * hd.ri : 0, hd.ri ? (mcus - k * hd.ri < hd.ri ? mcus - k * hd.ri : hd.ri) : mcus,
                                           k ? (k - 1) & 7 : -1};
            rows->insert(rows->end(), row, row + DH_SEG);
        }
        ++k;
        if (!rst) return k;
        first = p = q + 2;
    }
}

// ---- device -------------------------------------------------------------------------------------------------------------
struct Img {
    long long coef, out, qt;
    int W, H, nc, hs, vs;
    int bw[3], bh[3];
    long long comp_off[3];  // element offset of the component's blocks (and byte offset of its sample plane) from `coef`
};

// A descriptor is used only if everything it makes a kernel touch lies inside the buffers: the coefficient / plane range
// [coef, coef + blocks * 64) inside coef_elems, the tables inside qt_elems, the pixels inside out_bytes, and the grids
// large enough for the image (the Python layer passes what dbn_jpeg_entropy_batch wrote; a failed image has status != 0).
// Laxer than jpeg_common.h's read_scan on purpose: any grid that covers the image is taken, not only the derived one.
__device__ __forceinline__ bool load_img(const long long* __restrict__ d, long coef_elems, long qt_elems, long out_bytes, Img& g) {
    if (d[D_STATUS] != 0) return false;
    const long long W = d[D_W], H = d[D_H], nc = d[D_NC];
    if (W < 1 || H < 1 || W > 65535 || H > 65535 || (nc != 1 && nc != 3)) return false;
    g.W = (int)W, g.H = (int)H, g.nc = (int)nc;
    g.coef = d[D_COEF], g.out = d[D_OUT], g.qt = d[D_QT];
    const long long h0 = d[D_COMP + 2], v0 = d[D_COMP + 3];
    if (nc == 1) {
        g.hs = g.vs = 1;
    } else {
        if (!((h0 == 1 && v0 == 1) || (h0 == 2 && v0 == 1) || (h0 == 2 && v0 == 2))) return false;
        if (d[D_COMP + 6] != 1 || d[D_COMP + 7] != 1 || d[D_COMP + 10] != 1 || d[D_COMP + 11] != 1) return false;
        g.hs = (int)h0, g.vs = (int)v0;
    }
    long long blocks = 0;
    for (int c = 0; c < 3; ++c) {
        g.bw[c] = g.bh[c] = 0;
        g.comp_off[c] = blocks * 64;
        if (c >= nc) continue;
        const long long bw = d[D_COMP + 4 * c], bh = d[D_COMP + 4 * c + 1];
        const int cw = c == 0 ? g.W : (g.W + g.hs - 1) / g.hs, ch = c == 0 ? g.H : (g.H + g.vs - 1) / g.vs;
        if (bw < 1 || bh < 1 || bw > 16384 || bh > 16384 || bw * 8 < cw || bh * 8 < ch) return false;
        g.bw[c] = (int)bw, g.bh[c] = (int)bh;
        blocks += bw * bh;
    }
    if (nc == 3 && (g.bw[1] != g.bw[2] || g.bh[1] != g.bh[2])) return false;  // the chroma planes share one pitch
    if (g.coef < 0 || (g.coef & 63) || g.coef + blocks * 64 > coef_elems) return false;
    if (g.qt < 0 || (g.qt & 63) || g.qt + nc * 64 > qt_elems) return false;
    if (g.out < 0 || g.out + (long long)g.W * g.H * 3 > out_bytes) return false;
    return true;
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// jpeg_idct_islow's one-dimensional pass on eight values (CONST_BITS = 13); SHIFT 11 for columns, 18 for rows
template <int SHIFT>
__device__ __forceinline__ void idct_1d(const int (&i)[8], int (&o)[8]) {
    int z2 = i[2], z3 = i[6];
    int z1 = (z2 + z3) * 4433;
    int tmp2 = z1 + z3 * (-15137), tmp3 = z1 + z2 * 6270;
    int tmp0 = (int)((unsigned)(i[0] + i[4]) << 13), tmp1 = (int)((unsigned)(i[0] - i[4]) << 13);
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = i[7], tmp1 = i[5], tmp2 = i[3], tmp3 = i[1];
    z1 = tmp0 + tmp3, z2 = tmp1 + tmp2, z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * 9633;
    tmp0 *= 2446, tmp1 *= 16819, tmp2 *= 25172, tmp3 *= 12299;
    z1 *= -7373, z2 *= -20995, z3 = z3 * (-16069) + z5, z4 = z4 * (-3196) + z5;
    tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
    constexpr int R = 1 << (SHIFT - 1);
    o[0] = (tmp10 + tmp3 + R) >> SHIFT, o[7] = (tmp10 - tmp3 + R) >> SHIFT;
    o[1] = (tmp11 + tmp2 + R) >> SHIFT, o[6] = (tmp11 - tmp2 + R) >> SHIFT;
    o[2] = (tmp12 + tmp1 + R) >> SHIFT, o[5] = (tmp12 - tmp1 + R) >> SHIFT;
    o[3] = (tmp13 + tmp0 + R) >> SHIFT, o[4] = (tmp13 - tmp0 + R) >> SHIFT;
}

// ---- kernel 1: coefficients -> sample planes --------------------------------------------------------------------------------
// A workgroup takes ID_BLOCKS consecutive blocks of one component of one image (tab[wg] = {image, component, first block}); a
// wave takes eight of them, eight lanes per block.  Lane j of a block loads coefficient row j and table row j as one
// 16-byte vector each and multiplies; the products cross to the lanes as columns through LDS (block stride 72 dwords, row
// stride 9: neither the row-wise stores nor the column-wise loads meet a bank twice), lane j runs column j, the results
// cross back the same way, lane j runs row j and stores its eight samples as one 8-byte vector into the plane.
constexpr int ID_THREADS = 256, ID_BLOCKS = ID_THREADS / 8, ID_BSTRIDE = 72, ID_RSTRIDE = 9;
typedef short short8 __attribute__((ext_vector_type(8)));
typedef unsigned short ushort8 __attribute__((ext_vector_type(8)));

__global__ void __launch_bounds__(ID_THREADS) jpeg_idct_kernel(const short* __restrict__ coef, long coef_elems,
                                                                const long long* __restrict__ desc, int N,
                                                                const unsigned short* __restrict__ qtabs, long qt_elems,
                                                                const int* __restrict__ tab, long out_bytes,
                                                                unsigned char* __restrict__ planes) {
    __shared__ int s_t[ID_BLOCKS * ID_BSTRIDE];
    const int n = tab[4 * blockIdx.x], c = tab[4 * blockIdx.x + 1], blk0 = tab[4 * blockIdx.x + 2];
    Img g;
    bool ok = n >= 0 && n < N && c >= 0 && c < 3 && blk0 >= 0 && load_img(desc + (long)n * JP_DESC, coef_elems, qt_elems, out_bytes, g);
    ok = ok && c < g.nc;
    const int t = threadIdx.x, lb = t >> 3, j = t & 7;
    const long nblk = ok ? (long)g.bw[c] * g.bh[c] : 0;
    const long blk = (long)blk0 + lb;
    const bool live = ok && blk < nblk;
    int a[8], o[8];
    if (live) {
        const short8 k = *reinterpret_cast<const short8*>(coef + g.coef + g.comp_off[c] + blk * 64 + j * 8);
        const ushort8 q = *reinterpret_cast<const ushort8*>(qtabs + g.qt + c * 64 + j * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = (int)k[e] * (int)q[e];
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = 0;
    }
    int* sb = s_t + lb * ID_BSTRIDE;
#pragma unroll
    for (int e = 0; e < 8; ++e) sb[j * ID_RSTRIDE + e] = a[e];
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = sb[e * ID_RSTRIDE + j];  // column j
    idct_1d<11>(a, o);
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 8; ++e) sb[e * ID_RSTRIDE + j] = o[e];
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = sb[j * ID_RSTRIDE + e];  // row j
    idct_1d<18>(a, o);
    if (!live) return;
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        lo |= (unsigned)clamp255(o[e] + 128) << (8 * e);
        hi |= (unsigned)clamp255(o[e + 4] + 128) << (8 * e);
    }
    const long by = blk / g.bw[c], bx = blk - by * g.bw[c];
    unsigned char* dst = planes + g.coef + g.comp_off[c] + (by * 8 + j) * ((long)g.bw[c] * 8) + bx * 8;
    *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);
}

// ---- kernel 2: sample planes -> packed RGB -----------------------------------------------------------------------------------
// A workgroup owns RGB_PX consecutive pixels of one image's output run (tab[wg] = {image, chunk}; they may span rows), a lane
// four consecutive ones: it upsamples their chroma, converts, packs the twelve bytes into three dwords and puts them
// into LDS; the run then leaves as aligned dwords, with single bytes only at a run's unaligned ends (the packed layout
// gives an image's first byte any alignment).
constexpr int RGB_THREADS = 256, RGB_PPT = 4, RGB_PX = RGB_THREADS * RGB_PPT;

// one chroma sample at full-resolution (x, y): jdsample.c h2v1_fancy_upsample / h2v2_fancy_upsample over the true
// downsampled size cw x ch; fullsize for 1 x 1; replication when cw <= 2
__device__ __forceinline__ int chroma_at(const unsigned char* __restrict__ P, int pitch, int cw, int ch, int hs, int vs, int x, int y) {
    if (hs == 1) return P[(long)y * pitch + x];
    const int i = x >> 1, r = vs == 2 ? y >> 1 : y;
    const unsigned char* near = P + (long)r * pitch;
    if (cw <= 2) return near[i];
    const int odd = x & 1;
    const int i2 = odd ? i + 1 : i - 1;  // the other column, when inside
    const bool edge = i2 < 0 || i2 >= cw;
    if (vs == 1) {
        if (edge) return near[i];
        return (3 * near[i] + near[i2] + (odd ? 2 : 1)) >> 2;
    }
    int fr = (y & 1) ? r + 1 : r - 1;
    fr = fr < 0 ? 0 : (fr >= ch ? ch - 1 : fr);
    const unsigned char* far = P + (long)fr * pitch;
    const int t = 3 * near[i] + far[i];
    if (edge) return (4 * t + (odd ? 7 : 8)) >> 4;
    const int t2 = 3 * near[i2] + far[i2];
    return (3 * t + t2 + (odd ? 7 : 8)) >> 4;
}

__global__ void __launch_bounds__(RGB_THREADS) jpeg_rgb_kernel(const unsigned char* __restrict__ planes, long coef_elems,
                                                                const long long* __restrict__ desc, int N, long qt_elems,
                                                                const int* __restrict__ tab, unsigned char* __restrict__ out,
                                                                long out_bytes) {
    __shared__ unsigned int s_out[RGB_PX * 3 / 4];
    const int n = tab[4 * blockIdx.x], chunk = tab[4 * blockIdx.x + 1];
    Img g;
    if (!(n >= 0 && n < N && chunk >= 0 && load_img(desc + (long)n * JP_DESC, coef_elems, qt_elems, out_bytes, g))) return;
    const long npx = (long)g.W * g.H, p0 = (long)chunk * RGB_PX;
    if (p0 >= npx) return;
    const int t = threadIdx.x;
    const unsigned char* PY = planes + g.coef;
    const unsigned char* PB = PY + g.comp_off[1];
    const unsigned char* PR = PY + g.comp_off[2];
    const int pitchY = g.bw[0] * 8, pitchC = g.bw[1] * 8;
    const int cw = (g.W + g.hs - 1) / g.hs, ch = (g.H + g.vs - 1) / g.vs;
    const long q0 = p0 + (long)t * RGB_PPT;
    int y = (int)(q0 / g.W), x = (int)(q0 - (long)y * g.W);
    unsigned char px[12];
#pragma unroll
    for (int e = 0; e < RGB_PPT; ++e) {
        int r = 0, gg = 0, b = 0;
        if (q0 + e < npx) {
            const int Y = PY[(long)y * pitchY + x];
            if (g.nc == 1) {
                r = gg = b = Y;
            } else {
                const int cb = chroma_at(PB, pitchC, cw, ch, g.hs, g.vs, x, y) - 128;
                const int cr = chroma_at(PR, pitchC, cw, ch, g.hs, g.vs, x, y) - 128;
                r = clamp255(Y + ((91881 * cr + 32768) >> 16));
                gg = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
                b = clamp255(Y + ((116130 * cb + 32768) >> 16));
            }
        }
        px[3 * e] = (unsigned char)r, px[3 * e + 1] = (unsigned char)gg, px[3 * e + 2] = (unsigned char)b;
        if (++x == g.W) x = 0, ++y;
    }
#pragma unroll
    for (int w = 0; w < 3; ++w)
        s_out[t * 3 + w] = px[4 * w] | (unsigned)px[4 * w + 1] << 8 | (unsigned)px[4 * w + 2] << 16 | (unsigned)px[4 * w + 3] << 24;
    __syncthreads();
    const unsigned char* sb = reinterpret_cast<const unsigned char*>(s_out);
    const long b0 = p0 * 3;
    const int nb = (int)min((long)RGB_PX * 3, npx * 3 - b0);
    unsigned char* o = out + g.out + b0;
    const int head = (int)((4 - (reinterpret_cast<size_t>(o) & 3)) & 3);  // bytes before the first aligned dword
    const int lead = head < nb ? head : nb;
    const int nd = (nb - lead) >> 2, tail0 = lead + 4 * nd;
    if (t < lead) o[t] = sb[t];
    if (t >= 32 && t - 32 < nb - tail0) o[tail0 + t - 32] = sb[tail0 + t - 32];
    unsigned int* o4 = reinterpret_cast<unsigned int*>(o + lead);
    if (lead == 0) {
        for (int i = t; i < nd; i += RGB_THREADS) o4[i] = s_out[i];
    } else {
        for (int i = t; i < nd; i += RGB_THREADS) {
            const unsigned char* s = sb + lead + 4 * i;
            o4[i] = s[0] | (unsigned)s[1] << 8 | (unsigned)s[2] << 16 | (unsigned)s[3] << 24;
        }
    }
}

// ---- kernel 3: sample planes -> packed RGB, turned as the Exif orientation says -------------------------------------------------
// Output pixel (y', x') of an image with tag 2 .. 8 is source pixel (y, x): 2 (y', W-1-x'), 3 (H-1-y', W-1-x'), 4 (H-1-y', x'),
// 5 (x', y'), 6 (H-1-x', y'), 7 (H-1-x', W-1-y'), 8 (x', W-1-y'); the output is [W][H][3] for 5 .. 8.  The arithmetic per pixel is
// jpeg_rgb_kernel's in source coordinates, so the result is a permutation of the unoriented one.  A workgroup owns a TILE x TILE
// tile of the OUTPUT (tab[wg] = {image, tile row, tile column}), which is a TILE x TILE rectangle of the source as well.  Phase 1
// walks that rectangle in source order, a 32-lane half-wave along a source row (contiguous plane bytes), converts, and puts
// each pixel as one dword R | G << 8 | B << 16 at its OUTPUT place in LDS.  Phase 2 gives every output row segment (up to 96
// contiguous bytes) to one half-wave: lanes 0 .. 23 store the aligned dwords, lanes 24 .. 26 the bytes in front of the first
// aligned dword and lanes 27 .. 29 the bytes behind the last.  Pitch 33 dwords: in phase 1 the lanes of a half-wave write
// consecutive columns of one LDS row (tags 2 .. 4: stride 1 dword) or consecutive rows of one column (5 .. 8: stride 33, bank
// stride 1 of 32), in phase 2 they read distinct dwords of one row: no two lanes of a half-wave meet on a bank on either side.
constexpr int TILE = 32, TILE_PITCH = 33, TILE_THREADS = 256;

__global__ void __launch_bounds__(TILE_THREADS) jpeg_rgb_oriented_kernel(const unsigned char* __restrict__ planes, long coef_elems,
                                                                         const long long* __restrict__ desc, int N, long qt_elems,
                                                                         const int* __restrict__ orient, const int* __restrict__ tab,
                                                                         unsigned char* __restrict__ out, long out_bytes) {
    __shared__ unsigned int s_px[TILE * TILE_PITCH];
    const int n = tab[4 * blockIdx.x], ty = tab[4 * blockIdx.x + 1], tx = tab[4 * blockIdx.x + 2];
    Img g;
    if (!(n >= 0 && n < N && ty >= 0 && tx >= 0 && load_img(desc + (long)n * JP_DESC, coef_elems, qt_elems, out_bytes, g))) return;
    const int tag = orient[n];
    if (tag < 2 || tag > 8) return;
    const bool T = tag >= 5, fy = tag == 3 || tag == 4 || tag == 6 || tag == 7, fx = tag == 2 || tag == 3 || tag == 7 || tag == 8;
    const int OH = T ? g.W : g.H, OW = T ? g.H : g.W;
    if (ty > (OH - 1) / TILE || tx > (OW - 1) / TILE) return;
    const int y0 = ty * TILE, x0 = tx * TILE;
    const int th = min(TILE, OH - y0), tw = min(TILE, OW - x0);
    // the output rows run along the source's rows (a) or, transposed, along its columns; the source rectangle
    const int a0 = T ? x0 : y0, na = T ? tw : th, b0 = T ? y0 : x0, nb = T ? th : tw;
    const int sy0 = fy ? g.H - (a0 + na) : a0, sx0 = fx ? g.W - (b0 + nb) : b0;
    const int t = threadIdx.x, lx = t & 31;
    const unsigned char* PY = planes + g.coef;
    const unsigned char* PB = PY + g.comp_off[1];
    const unsigned char* PR = PY + g.comp_off[2];
    const int pitchY = g.bw[0] * 8, pitchC = g.bw[1] * 8;
    const int cw = (g.W + g.hs - 1) / g.hs, ch = (g.H + g.vs - 1) / g.vs;
#pragma unroll
    for (int i = 0; i < TILE * TILE / TILE_THREADS; ++i) {
        const int ly = (t >> 5) + i * (TILE_THREADS / 32);
        if (ly < na && lx < nb) {
            const int y = sy0 + ly, x = sx0 + lx;
            const int Y = PY[(long)y * pitchY + x];
            int r = Y, gg = Y, b = Y;
            if (g.nc != 1) {
                const int cb = chroma_at(PB, pitchC, cw, ch, g.hs, g.vs, x, y) - 128;
                const int cr = chroma_at(PR, pitchC, cw, ch, g.hs, g.vs, x, y) - 128;
                r = clamp255(Y + ((91881 * cr + 32768) >> 16));
                gg = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
                b = clamp255(Y + ((116130 * cb + 32768) >> 16));
            }
            const int la = fy ? na - 1 - ly : ly, lb = fx ? nb - 1 - lx : lx;
            const int oy = T ? lb : la, ox = T ? la : lb;
            s_px[oy * TILE_PITCH + ox] = (unsigned)r | (unsigned)gg << 8 | (unsigned)b << 16;
        }
    }
    __syncthreads();
    const int seg = tw * 3;  // bytes of a row segment
#pragma unroll
    for (int i = 0; i < TILE * TILE / TILE_THREADS; ++i) {
        const int row = (t >> 5) + i * (TILE_THREADS / 32);
        if (row >= th) continue;
        unsigned char* o = out + g.out + ((long)(y0 + row) * OW + x0) * 3;
        const int head = (int)((4 - (reinterpret_cast<size_t>(o) & 3)) & 3);
        const int lead = head < seg ? head : seg;
        const int nd = (seg - lead) >> 2, tail0 = lead + 4 * nd;
        const unsigned int* sr = s_px + row * TILE_PITCH;
        if (lx < 24) {
            if (lx < nd) {
                const int q = lead + 4 * lx, a = q / 3, sh = 8 * (q - 3 * a);  // bytes q .. q + 3 lie in pixels a and a + 1 (a + 1 < tw: q + 3 < seg)
                const unsigned long long v = (unsigned long long)sr[a] | (unsigned long long)sr[a + 1] << 24;
                reinterpret_cast<unsigned int*>(o + lead)[lx] = (unsigned int)(v >> sh);
            }
        } else if (lx < 30) {
            const int k = lx < 27 ? lx - 24 : lx - 27;
            const int q = lx < 27 ? k : tail0 + k;
            if (lx < 27 ? k < lead : q < seg) o[q] = (unsigned char)(sr[q / 3] >> (8 * (q % 3)));
        }
    }
}

}  // namespace

extern "C" {

// out[24]: 0 status (support code), 1 width, 2 height, 3 components, 4 restart interval, 5 Exif orientation (0 none),
// 6 + 2c / 7 + 2c sampling factors h / v of component c (c < 4), 14 SOF type (0 baseline, 1 extended, 2 progressive; -1 unknown),
// 15 int16 coefficients the stream needs (0 unless supported), 16 JFIF marker seen, 17 Adobe transform (-1 no marker),
// 18 sample precision, 19 scans (counted by their markers; 0 unless supported, and without JF_MULTISCAN)
int dbn_jpeg_info_ex(const unsigned char* data, long len, int flags, long long* out) {
    DBN_REQUIRE(data && out && len >= 0);
    Header* hd = new Header;
    parse_header(data, len, *hd, flags);
    for (int i = 0; i < JP_INFO; ++i) out[i] = 0;
    out[0] = hd->status, out[1] = hd->width, out[2] = hd->height, out[3] = hd->ncomp, out[4] = hd->ri, out[5] = hd->orientation;
    for (int c = 0; c < 4; ++c) out[6 + 2 * c] = hd->h[c], out[7 + 2 * c] = hd->v[c];
    out[14] = hd->sof, out[15] = hd->status == JS_OK ? hd->coef_elems() : 0, out[16] = hd->jfif, out[17] = hd->adobe;
    out[18] = hd->precision;
    if ((flags & JF_MULTISCAN) && hd->status == JS_OK) out[19] = hd->multi ? count_scans(data, len, hd->sos_at) : 1;
    delete hd;
    return DBN_OK;
}

int dbn_jpeg_info(const unsigned char* data, long len, long long* out) { return dbn_jpeg_info_ex(data, len, 0, out); }

// per_image[n] = int16 coefficients of stream n = blob[offs[n] .. offs[n + 1]) (0 for one that cannot be decoded); the sum
long dbn_jpeg_coef_elems_ex(const unsigned char* blob, const long long* offs, int N, int flags, long long* per_image) {
    if (!blob || !offs || N < 0) return -1;
    long total = 0;
    Header* hd = new Header;
    for (int n = 0; n < N; ++n) {
        *hd = Header();
        long e = 0;
        if (offs[n] >= 0 && offs[n + 1] >= offs[n]) {
            parse_header(blob + offs[n], (long)(offs[n + 1] - offs[n]), *hd, flags);
            if (hd->status == JS_OK) e = hd->coef_elems();
        }
        if (per_image) per_image[n] = e;
        total += e;
    }
    delete hd;
    return total;
}

long dbn_jpeg_coef_elems(const unsigned char* blob, const long long* offs, int N, long long* per_image) {
    return dbn_jpeg_coef_elems_ex(blob, offs, N, 0, per_image);
}

// coef: coef_elems int16 (dbn_jpeg_coef_elems_ex with the same flags); desc: int64 [N][24]; qtabs: uint16 [N][3][64] (natural order,
// one table per component); status: int [N]; orientation (may be null): int [N], the Exif tag of every header, 0 none.  Image n's
// coefficients start at the sum of the counts before it, its pixels at the sum of the H * W * 3 of the decodable headers before it.
// An image whose scan fails keeps its slots (zeroed) and a status != 0.  JF_MULTISCAN: progressive streams and sequential ones
// of several scans are decoded too (decode_scans); their descriptor's restart interval is the one in force at the first scan.
int dbn_jpeg_entropy_batch_ex(const unsigned char* blob, const long long* offs, int N, short* coef, long coef_elems, long long* desc,
                              unsigned short* qtabs, int* status, int* orientation, int threads, int flags) {
    DBN_REQUIRE(blob && offs && desc && qtabs && status && N > 0 && coef_elems >= 0 && (coef || coef_elems == 0));
    for (int n = 0; n < N; ++n) DBN_REQUIRE(offs[n] >= 0 && offs[n + 1] >= offs[n]);
    std::vector<Header> hds((size_t)N);
    long co = 0, oo = 0;
    for (int n = 0; n < N; ++n) {
        Header& hd = hds[n];
        parse_header(blob + offs[n], (long)(offs[n + 1] - offs[n]), hd, flags);
        status[n] = hd.status;
        if (orientation) orientation[n] = hd.orientation;
        if (!describe(hd, n, coef_elems, co, oo, desc + (long)n * JP_DESC, qtabs + (long)n * 192)) return DBN_ERR_ARG;
    }
    on_threads(N, threads, [&](int n) {
        Header& hd = hds[n];
        if (hd.status != JS_OK) return;
        long long* d = desc + (long)n * JP_DESC;
        const unsigned char* data = blob + offs[n];
        const long len = (long)(offs[n + 1] - offs[n]);
        const int s = hd.multi ? decode_scans(data, len, hd, coef + d[D_COEF], nullptr) : decode_scan(data, len, hd, coef + d[D_COEF]);
        if (s != JS_OK) {
            memset(coef + d[D_COEF], 0, (size_t)hd.coef_elems() * sizeof(short));
            d[D_STATUS] = status[n] = s;
        } else if (hd.multi) {
            memcpy(qtabs + (long)n * 192, hd.cqt, (size_t)hd.ncomp * 64 * sizeof(unsigned short));
        }
    });
    return DBN_OK;
}

int dbn_jpeg_entropy_batch(const unsigned char* blob, const long long* offs, int N, short* coef, long coef_elems, long long* desc,
                           unsigned short* qtabs, int* status, int threads) {
    return dbn_jpeg_entropy_batch_ex(blob, offs, N, coef, coef_elems, desc, qtabs, status, nullptr, threads, 0);
}

// coef / desc / qtabs: the outputs of dbn_jpeg_entropy_batch, on the device; tab_idct int32 [n_idct][4] = {image, component,
// first block, 0} (one workgroup per 32 blocks), tab_rgb int32 [n_rgb][4] = {image, chunk of 1024 pixels, 0, 0}; planes: a
// workspace of coef_elems bytes; out: out_bytes bytes, every pixel of every image with status 0 written once.
// orientation int32 [N] (device) and tab_tile int32 [n_tile][4] = {image, tile row, tile column, 0} over the 32 x 32 tiles of the
// ORIENTED image: the images whose tag is 2 .. 8, which the host lists there and not in tab_rgb, are written turned
// (jpeg_rgb_oriented_kernel), as [W][H][3] for tags 5 .. 8.  Either table may be empty (its pointers are then not read).
int dbn_jpeg_pixels_ex(const short* coef, long coef_elems, const long long* desc, const unsigned short* qtabs, int N, const int* tab_idct,
                       int n_idct, const int* tab_rgb, int n_rgb, const int* orientation, const int* tab_tile, int n_tile,
                       unsigned char* planes, unsigned char* out, long out_bytes, void* stream) {
    DBN_REQUIRE(coef && desc && qtabs && tab_idct && planes && out && N > 0 && n_idct > 0 && n_rgb >= 0 && n_tile >= 0 && n_rgb + n_tile > 0 &&
                coef_elems > 0 && out_bytes > 0);
    DBN_REQUIRE((n_rgb == 0 || tab_rgb) && (n_tile == 0 || (tab_tile && orientation)));
    DBN_REQUIRE((reinterpret_cast<size_t>(coef) & 15) == 0 && (reinterpret_cast<size_t>(qtabs) & 15) == 0 &&
                (reinterpret_cast<size_t>(planes) & 7) == 0);
    const long qt_elems = (long)N * 192;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)n_idct), dim3(ID_THREADS), 0, (hipStream_t)stream, coef, coef_elems, desc, N, qtabs,
                       qt_elems, tab_idct, out_bytes, planes);
    if (n_rgb)
        hipLaunchKernelGGL(jpeg_rgb_kernel, dim3((unsigned)n_rgb), dim3(RGB_THREADS), 0, (hipStream_t)stream, planes, coef_elems, desc, N, qt_elems,
                           tab_rgb, out, out_bytes);
    if (n_tile)
        hipLaunchKernelGGL(jpeg_rgb_oriented_kernel, dim3((unsigned)n_tile), dim3(TILE_THREADS), 0, (hipStream_t)stream, planes, coef_elems, desc, N,
                           qt_elems, orientation, tab_tile, out, out_bytes);
    return dbn_status();
}

int dbn_jpeg_pixels(const short* coef, long coef_elems, const long long* desc, const unsigned short* qtabs, int N, const int* tab_idct,
                    int n_idct, const int* tab_rgb, int n_rgb, unsigned char* planes, unsigned char* out, long out_bytes, void* stream) {
    DBN_REQUIRE(tab_rgb && n_rgb > 0);
    return dbn_jpeg_pixels_ex(coef, coef_elems, desc, qtabs, N, tab_idct, n_idct, tab_rgb, n_rgb, nullptr, nullptr, 0, planes, out, out_bytes, stream);
}

// The host half of the device entropy stage: headers as dbn_jpeg_entropy_batch parses them (same kinds, same status
// codes), and the scans cut at their markers.  desc / qtabs / status: as dbn_jpeg_entropy_batch writes them, for headers
// alone (what is wrong inside a scan is found later, by the device or by the host decoder it falls back to).  hspec uint8
// [N][8][273], info int64 [N][8], seg int64 [seg_cap][6], sub_base int64 [seg_cap + 1] (first subsequence of each segment,
// numbered over the batch), wgtab int32 [wg_cap][4] = {image, first subsequence, count, 0}: csrc/jpeg_dhuff.h.  seg ==
// nullptr counts only.  counts int64 [4] = {segments, subsequences, workgroups, int16 coefficients}.
int dbn_jpeg_stream_plan(const unsigned char* blob, const long long* offs, int N, long long* desc, unsigned short* qtabs, int* status,
                         unsigned char* hspec, long long* info, long long* seg, long seg_cap, long long* sub_base, int* wgtab, long wg_cap,
                         long long* counts) {
    using namespace dbn_dhuff;
    DBN_REQUIRE(blob && offs && desc && qtabs && status && hspec && info && counts && N > 0);
    DBN_REQUIRE(!seg || (sub_base && wgtab && seg_cap >= 0 && wg_cap >= 0));
    for (int n = 0; n < N; ++n) DBN_REQUIRE(offs[n] >= 0 && offs[n + 1] >= offs[n]);
    Header* hd = new Header;
    std::vector<long long> rows;
    long co = 0, oo = 0, nseg = 0, nsub = 0, nwg = 0;
    int rc = DBN_OK;
    for (int n = 0; n < N && rc == DBN_OK; ++n) {
        *hd = Header();
        const unsigned char* d = blob + offs[n];
        const long len = (long)(offs[n + 1] - offs[n]);
        parse_header(d, len, *hd);
        status[n] = hd->status;
        describe(*hd, n, co + hd->coef_elems(), co, oo, desc + (long)n * JP_DESC, qtabs + (long)n * 192);
        unsigned char* hs = hspec + (long)n * 8 * DH_SPEC;
        memset(hs, 0, 8 * DH_SPEC);
        long long* in = info + (long)n * DH_INFO;
        for (int i = 0; i < DH_INFO; ++i) in[i] = 0;
        in[DI_BEGIN] = offs[n], in[DI_END] = offs[n + 1], in[DI_SEG0] = nseg, in[DI_SUB0] = nsub;
        if (hd->status != JS_OK) continue;
        for (int t = 0; t < 8; ++t) {
            const Huff& h = t < 4 ? hd->dc[t] : hd->ac[t - 4];
            if (!h.present) continue;
            unsigned char* s = hs + t * DH_SPEC;
            s[0] = 1;
            for (int l = 1; l <= 16; ++l) s[l] = (unsigned char)(h.maxcode[l] >= 0 ? h.maxcode[l] - h.mincode[l] + 1 : 0);
            memcpy(s + 17, h.vals, (size_t)h.nvals);
        }
        for (int c = 0; c < hd->ncomp; ++c) in[DI_SEL] |= (long long)(hd->td[c] | hd->ta[c] << 4) << (8 * c);
        rows.clear();
        const long k = scan_segments(d, len, *hd, &rows);
        if (k < 0) {
            in[DI_HOST] = 1;
            continue;
        }
        long subs = 0;
        for (long i = 0; i < k; ++i) {
            long long* r = rows.data() + i * DH_SEG;
            const long bits = (long)(r[SG_END] - r[SG_FIRST]) * 8;
            const long ns = bits ? (bits + DH_S - 1) / DH_S : 1;
            if (seg) {
                if (nseg + i >= seg_cap) {
                    rc = DBN_ERR_ARG;
                    break;
                }
                long long* o = seg + (nseg + i) * DH_SEG;
                memcpy(o, r, sizeof(long long) * DH_SEG);
                o[SG_IMAGE] = n, o[SG_FIRST] += offs[n], o[SG_END] += offs[n];
                sub_base[nseg + i] = nsub + subs;
            }
            subs += ns;
        }
        const long wgs = (subs + DH_THREADS - 1) / DH_THREADS;
        if (seg && rc == DBN_OK) {
            if (nwg + wgs > wg_cap) rc = DBN_ERR_ARG;
            for (long w = 0; w < wgs && rc == DBN_OK; ++w) {
                int* o = wgtab + (nwg + w) * 4;
                o[0] = n, o[1] = (int)(nsub + w * DH_THREADS), o[2] = (int)(subs - w * DH_THREADS < DH_THREADS ? subs - w * DH_THREADS : DH_THREADS), o[3] = 0;
            }
        }
        in[DI_NSEG] = k, in[DI_NSUB] = subs;
        nseg += k, nsub += subs, nwg += wgs;
        if (nsub > 0x7FFFFF00L) rc = DBN_ERR_ARG;
    }
    delete hd;
    if (seg && rc == DBN_OK) sub_base[nseg] = nsub;
    counts[0] = nseg, counts[1] = nsub, counts[2] = nwg, counts[3] = co;
    return rc;
}

}  // extern "C"
