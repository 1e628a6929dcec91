// What the two halves of the JPEG encode share (jpeg_enc.hip: device forward stage and host Huffman stage; jpeg_huff.hip: the
// device Huffman stage): the status codes, the host coder's geometry, a Huffman table as a DHT segment holds it, and the host
// functions that build tables and write a stream's header.  The descriptor and its checks are jpeg_common.h's.
#pragma once

#include "jpeg_common.h"

namespace dbn_jpeg {

enum { ES_OK = 0, ES_NO_IMAGE, ES_BAD_DESC, ES_TABLE, ES_DC_RANGE, ES_AC_RANGE, ES_NO_ROOM, ES_CODE_LENGTH };

constexpr long kHeaderBytes = 704;  // SOI 2, APP0 18, 3 DQT 207, SOF0 19, 4 DHT 432, DRI 6, SOS 14, EOI 2
// A block takes at most 9 + 11 bits of DC and 63 x (16 + 10) bits of AC: 208 bytes, every one of which may be FF and stuffed.
constexpr long kBlockBits = 20 + 63 * 26, kBlockBytes = 416;

// what the host stage needs of a descriptor: read_scan's result per component (walk_scan and the header index them), and the tables
struct Geo {
    int W, H, nc, mcux, mcuy, h[3], v[3], bw[3], bh[3];
    long coef, qt, comp_off[3], blocks;
};
int load_geo(const long long* d, long coef_elems, long qt_elems, Geo& g);

// a table as its DHT segment holds it: symbols per code length 1 .. 16, then the symbols by length and value
struct HuffSpec {
    unsigned char bits[16];
    unsigned char vals[256];
    int nvals;
};

struct Codes {
    unsigned short code[256];
    unsigned char size[256];  // 0: no code for this symbol
    Codes() {}
    Codes(const unsigned char* bits, const unsigned char* vals);
};

// the Annex K.3 tables, in the order of an image's tables everywhere here: DC 0, AC 0, DC 1, AC 1
const HuffSpec* annex_k();
// libjpeg's jpeg_gen_optimal_table for the counts freq[0 .. 255]; ES_OK, or ES_CODE_LENGTH where libjpeg gives up (a code of more than 32 bits)
int optimal_table(const long long* freq, HuffSpec& out);
// SOI .. SOS of one image into [out, out + room) -> bytes written, -1 if they do not fit; ES_TABLE's check is the caller's
long write_header(const unsigned short* qtabs, const Geo& g, int ri, const HuffSpec* specs, unsigned char* out, long room);
// ES_OK, or ES_TABLE for a quantisation value outside 1 .. 255
int check_qtabs(const unsigned short* qtabs, const Geo& g);

}  // namespace dbn_jpeg
