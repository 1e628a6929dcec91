// Edit distances between strings of classes, on the device: the scoring and lexicon-correction step behind the reader of
// csrc/recognise.hip (db_text_minimal_amd/spotting.py).
//   edit_distance_pairs   P independent (pattern, text) pairs -> dist[P], one wave per pair
//   lexicon_nearest       K queries against a lexicon resident on the device -> the nearest entry and its distance, one
//                         lane per lexicon entry
//
// Strings are bytes of classes 0 .. 254; class 255 matches nothing, not even itself.  The distance is the unit-cost
// Levenshtein distance (insert, delete, substitute), exact in integers.  Both kernels run the Myers / Hyyro bit-vector
// recurrence with the pattern (m <= 64 classes) in one 64-bit word: column j of the DP table is the pair of bit vectors
// (Pv, Mv) of its +1 / -1 vertical differences, `score` is its last cell.
//   Pv = ~0, Mv = 0, score = m, top = 1 << (m - 1); per text class c with Eq = the positions of the pattern that hold c:
//     Xv = Eq | Mv;  Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;  Ph = Mv | ~(Xh | Pv);  Mh = Pv & Xh
//     score += (Ph & top) != 0;  score -= (Mh & top) != 0
//     Ph = (Ph << 1) | 1;  Mh <<= 1;  Pv = Mh | ~(Xv | Ph);  Mv = Ph & Xv
// Bits at and above m never reach bit m - 1 (the carry of the sum and the shifts move upwards only), so they need no mask.
// m = 0 gives the text's length.
//
// The two kernels build Eq differently on purpose, so that each checks the other:
//   pairs     lane j of the wave holds pattern class j; Eq is the 64-bit ballot of `pattern[lane] == c` over the wave, and
//             the update is uniform (scalar) across the wave.  No table.
//   nearest   the QUERY is the pattern: a workgroup builds its table Peq[256] (one 64-bit word per class, 2 KB of LDS) once
//             -- thread c forms word c from the query's bytes, so every word is written (zero where the class does not
//             occur, and for class 255) and no zeroing pass or LDS atomic is needed -- and every lane runs the recurrence
//             over one lexicon entry with Eq = Peq[c].
//
// Lexicon layout.  Entries are ordered by (group, length) and cut into blocks of 64; a group starts on a block boundary.
// Block b holds rows_b positions (the longest entry of the block, rounded up to a multiple of four) of 64 bytes each,
// position-major: byte blk_off[b] + pos * 64 + lane is class `pos` of the block's entry `lane`, so a wave's load of one
// position reads 64 consecutive bytes, and its lanes run similar trip counts.  ent_len[b * 64 + lane] is the entry's length
// (-1: a padding slot), ent_idx[...] its index in the caller's order within its group.
//
// Tie rule.  A lane's key is (distance << 32) | original index; the wave takes the minimum, one lane folds it into the
// query's 64-bit slot of the workspace with one atomicMin (a vector global atomic).  The entry point makes three launches:
// one sets the slots to all-ones, one searches, one splits the slots into index[K] and dist[K].  The minimum of that key is the smallest distance and, among equals, the smallest original
// index, whatever the order of execution: two runs agree in every bit.
#include "common.h"

namespace {

constexpr int LX_THREADS = 256, LX_WAVES = LX_THREADS / 64;
constexpr int LX_MAX_TILES = 16;  // workgroups that share one query's group (each builds the query's table once)
constexpr unsigned long long LX_NONE = ~0ull;

struct Myers {
    unsigned long long Pv, Mv, top;
    int score;
    __device__ __forceinline__ void init(int m) { Pv = ~0ull, Mv = 0ull, top = 1ull << (m - 1), score = m; }  // m in 1 .. 64
    __device__ __forceinline__ void step(unsigned long long Eq) {
        const unsigned long long Xv = Eq | Mv;
        const unsigned long long Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
        unsigned long long Ph = Mv | ~(Xh | Pv);
        unsigned long long Mh = Pv & Xh;
        score += (Ph & top) != 0ull;
        score -= (Mh & top) != 0ull;
        Ph = (Ph << 1) | 1ull;
        Mh <<= 1;
        Pv = Mh | ~(Xv | Ph);
        Mv = Ph & Xv;
    }
};

// ---- pairs: one wave per pair ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(LX_THREADS) edit_distance_pairs_kernel(const unsigned char* __restrict__ pattern, int T, const int* __restrict__ pat_len,
                                                                          const unsigned char* __restrict__ text, long n_text,
                                                                          const int* __restrict__ text_off, const int* __restrict__ text_len, int P,
                                                                          int* __restrict__ dist) {
    const long p = (long)blockIdx.x * LX_WAVES + (threadIdx.x >> 6);
    if (p >= P) return;
    const int lane = threadIdx.x & 63;
    int m = pat_len[p];
    m = m < 0 ? 0 : (m > T ? T : m);
    // the text's bytes [o0, o0 + n) lie within [0, n_text) whatever the tables hold
    long o0 = text_off[p];
    o0 = o0 < 0 ? 0 : (o0 > n_text ? n_text : o0);
    long n = text_len ? (long)text_len[p] : (long)text_off[p + 1] - o0;
    n = n < 0 ? 0 : (n > n_text - o0 ? n_text - o0 : n);
    int d;
    if (m == 0) {
        d = (int)n;
    } else {
        const int pc = lane < m ? (int)pattern[p * T + lane] : 255;  // 255 matches nothing
        Myers s;
        s.init(m);
        for (long base = 0; base < n; base += 64) {
            const int cnt = n - base < 64 ? (int)(n - base) : 64;
            const int ch = lane < cnt ? (int)text[o0 + base + lane] : 255;
            for (int i = 0; i < cnt; ++i) {
                const int c = __shfl(ch, i, 64);
                s.step(__ballot(pc == c && c != 255));
            }
        }
        d = s.score;
    }
    if (lane == 0) dist[p] = d;
}

// ---- nearest: one lane per lexicon entry ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(LX_THREADS) lexicon_init_kernel(unsigned long long* __restrict__ slot, int K) {
    const long k = (long)blockIdx.x * LX_THREADS + threadIdx.x;
    if (k < K) slot[k] = LX_NONE;
}

__global__ void __launch_bounds__(LX_THREADS) lexicon_nearest_kernel(const unsigned char* __restrict__ query, int T, const int* __restrict__ qlen,
                                                                      const int* __restrict__ group, const unsigned char* __restrict__ data,
                                                                      const int* __restrict__ blk_off, const int* __restrict__ ent_len,
                                                                      const int* __restrict__ ent_idx, const int* __restrict__ grp_blk, int G, int NB,
                                                                      unsigned long long* __restrict__ slot) {
    __shared__ unsigned long long s_peq[256];
    __shared__ unsigned char s_q[64];
    const int k = blockIdx.x, t = threadIdx.x;
    const int g = group ? group[k] : 0;
    if (g < 0 || g >= G) return;  // (uniform over the workgroup)
    int b0 = grp_blk[g], b1 = grp_blk[g + 1];
    b0 = b0 < 0 ? 0 : b0;
    b1 = b1 > NB ? NB : b1;
    const int first = b0 + (int)blockIdx.y * LX_WAVES;
    if (first >= b1) return;  // an empty group, or a tile beyond this group's blocks
    int m = qlen[k];
    m = m < 0 ? 0 : (m > T ? T : m);
    if (t < 64) s_q[t] = t < m ? query[(long)k * T + t] : 255;
    __syncthreads();
    {
        unsigned long long w = 0ull;
        if (t != 255)
            for (int j = 0; j < m; ++j) w |= (unsigned long long)(s_q[j] == t) << j;
        s_peq[t] = w;
    }
    __syncthreads();
    const int lane = t & 63, stride = (int)gridDim.y * LX_WAVES;
    unsigned long long best = LX_NONE;
    for (int b = first + (t >> 6); b < b1; b += stride) {
        const int e = b * 64 + lane;
        const int L = ent_len[e];
        if (L < 0) continue;  // a padding slot
        int d;
        if (m == 0) {
            d = L;
        } else {
            const unsigned char* col = data + blk_off[b] + lane;
            Myers s;
            s.init(m);
            for (int pos = 0; pos < L; pos += 4) {  // the block's rows are a multiple of four: all four loads stay inside it
                const int c0 = col[pos * 64], c1 = col[(pos + 1) * 64], c2 = col[(pos + 2) * 64], c3 = col[(pos + 3) * 64];
                s.step(s_peq[c0]);
                if (pos + 1 < L) s.step(s_peq[c1]);
                if (pos + 2 < L) s.step(s_peq[c2]);
                if (pos + 3 < L) s.step(s_peq[c3]);
            }
            d = s.score;
        }
        const unsigned long long key = ((unsigned long long)(unsigned)d << 32) | (unsigned)ent_idx[e];
        best = key < best ? key : best;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned hi = (unsigned)__shfl_xor((int)(best >> 32), o, 64), lo = (unsigned)__shfl_xor((int)(best & 0xFFFFFFFFull), o, 64);
        const unsigned long long other = ((unsigned long long)hi << 32) | lo;
        best = other < best ? other : best;
    }
    if (lane == 0 && best != LX_NONE) atomicMin(&slot[k], best);
}

__global__ void __launch_bounds__(LX_THREADS) lexicon_split_kernel(const unsigned long long* __restrict__ slot, int K, int* __restrict__ index,
                                                                    int* __restrict__ dist) {
    const long k = (long)blockIdx.x * LX_THREADS + threadIdx.x;
    if (k >= K) return;
    const unsigned long long key = slot[k];
    index[k] = key == LX_NONE ? -1 : (int)(key & 0xFFFFFFFFull);
    dist[k] = key == LX_NONE ? -1 : (int)(key >> 32);
}

}  // namespace

extern "C" {

int dbn_edit_distance_pairs(const unsigned char* pattern, int T, const int* pat_len, const unsigned char* text, long n_text, const int* text_off,
                            const int* text_len, int P, int* dist, void* stream) {
    DBN_REQUIRE(pattern && pat_len && text_off && dist && P > 0 && T >= 1 && T <= 64 && n_text >= 0 && (text || n_text == 0));
    const int blocks = (int)(((long)P + LX_WAVES - 1) / LX_WAVES);
    hipLaunchKernelGGL(edit_distance_pairs_kernel, dim3((unsigned)blocks), dim3(LX_THREADS), 0, (hipStream_t)stream, pattern, T, pat_len, text, n_text,
                       text_off, text_len, P, dist);
    return dbn_status();
}

long dbn_lexicon_ws_bytes(int K) { return K > 0 ? (long)K * 8 : 0; }

int dbn_lexicon_nearest(const unsigned char* query, int T, const int* qlen, const int* group, int K, const unsigned char* data, const int* blk_off,
                        const int* ent_len, const int* ent_idx, const int* grp_blk, int G, int NB, int max_blocks, void* ws, int* index, int* dist,
                        void* stream) {
    DBN_REQUIRE(query && qlen && ws && index && dist && K > 0 && T >= 1 && T <= 64 && G >= 1 && NB >= 0 && max_blocks >= 0 && max_blocks <= NB);
    DBN_REQUIRE(grp_blk && (NB == 0 || (data && blk_off && ent_len && ent_idx)) && (reinterpret_cast<size_t>(ws) & 7) == 0);
    unsigned long long* slot = reinterpret_cast<unsigned long long*>(ws);
    hipStream_t st = (hipStream_t)stream;
    const int flat = (int)(((long)K + LX_THREADS - 1) / LX_THREADS);
    hipLaunchKernelGGL(lexicon_init_kernel, dim3((unsigned)flat), dim3(LX_THREADS), 0, st, slot, K);
    if (max_blocks > 0) {
        int tiles = (max_blocks + LX_WAVES - 1) / LX_WAVES;
        tiles = tiles > LX_MAX_TILES ? LX_MAX_TILES : tiles;
        hipLaunchKernelGGL(lexicon_nearest_kernel, dim3((unsigned)K, (unsigned)tiles), dim3(LX_THREADS), 0, st, query, T, qlen, group, data, blk_off,
                           ent_len, ent_idx, grp_blk, G, NB, slot);
    }
    hipLaunchKernelGGL(lexicon_split_kernel, dim3((unsigned)flat), dim3(LX_THREADS), 0, st, slot, K, index, dist);
    return dbn_status();
}

}  // extern "C"
