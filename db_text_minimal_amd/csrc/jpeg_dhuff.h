// What the host plan (dbn_jpeg_stream_plan, jpeg.hip) and the device Huffman decoder (jpeg_dhuff.hip) agree on: the layout of
// the plan.  The descriptor, its checks and the canonical Huffman code ranges both use are jpeg_common.h's.
#pragma once

namespace dbn_dhuff {

constexpr int DH_S = 1024;       // bits of (stuffed) entropy data per subsequence: one lane's share
constexpr int DH_THREADS = 256;  // lanes, and so subsequences, per workgroup
constexpr int DH_MAX_ROUNDS = 64;

// segment table: int64 [segments][6]; bytes are offsets into the blob, `end` is the FF of the marker behind the segment
constexpr int DH_SEG = 6;
enum { SG_IMAGE = 0, SG_FIRST, SG_END, SG_MCU0, SG_MCUS, SG_RST /* n of the RSTn in front of it, -1 for an image's first */ };

// per image: int64 [N][8]
constexpr int DH_INFO = 8;
enum {
    DI_SEL = 0,  // Huffman table of component c: DC id in bits 8c .. 8c + 3, AC id in bits 8c + 4 .. 8c + 7
    DI_HOST,     // 1: the markers of the scan are not the ones the header calls for; the host decoder decides what it is
    DI_BEGIN, DI_END,  // the stream's bytes in the blob
    DI_SEG0, DI_NSEG,  // its rows of the segment table
    DI_SUB0, DI_NSUB   // its subsequences, numbered over the batch
};

// Huffman table specs: uint8 [N][8][273], DC 0 .. 3 then AC 0 .. 3; per table {present, 16 counts, 256 values}
constexpr int DH_SPEC = 273;

}  // namespace dbn_dhuff
