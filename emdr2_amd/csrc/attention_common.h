// emdr2_amd/csrc/attention_common.h -- tile layout and fragment helpers shared by the fused attention kernels (attention.hip,
// attention_bwd.hip).  Tiles are [64 rows][64 d] bf16 (128-B rows of eight 16-B granules) filled by LDS-DMA with the granule index XOR
// f(row), f(row) = (((row >> 1) & 1) << 2) | ((row >> 2) & 3): conflict-free both for row reads (ds_read_b128: 16 consecutive rows, one
// granule) and for ds_read_b64_tr_b16 transpose reads (4 rows x 4 granules per 32-lane service group; layout pinned by tools/tr_probe.hip).
#ifndef EMDR2_ATTENTION_COMMON_H
#define EMDR2_ATTENTION_COMMON_H
#include <type_traits>
#include "prims.h"

#define L2E 1.4426950408889634f
#define MASKED2 (-10000.f * 1.4426950408889634f)

__device__ __forceinline__ int tile_swz(int row) { return (((row >> 1) & 1) << 2) | ((row >> 2) & 3); }

// Fragment of the row-major global matrix row: 8 bf16 at d = 16 t + 8 hi for t = 0..3 (the B operand of the "swapped" MFMAs)
__device__ __forceinline__ void load_row_frags(const char *row, int hi, bf16x8 (&f)[4])
{
#pragma unroll
    for (int t = 0; t < 4; ++t) f[t] = *(const bf16x8 *)(row + (16 * t + 8 * hi) * 2);
}

// Row fragment (MFMA A operand, 8 consecutive d of one tile row) from a swizzled tile
__device__ __forceinline__ bf16x8 tile_row_frag(const char *tile, int row, int gran)
{
    return *(const bf16x8 *)(tile + row * 128 + ((gran ^ tile_swz(row)) << 4));
}

// The same row fragments by inline asm, for the kernels that have an LDS-DMA in flight while they read (all of them: the next block is
// staged while this one is consumed).  For a plain load from the staging buffer the compiler's wait-count pass assumes it may alias the DMA
// destination and puts s_waitcnt vmcnt(0) in front of it: the prefetch of the next block was waited for BEFORE the current block was touched
// and the double buffering hid nothing.  row_frag_addresses: the lane's byte address (row = lane & 31, stage 0) for k-step t = 0..3; the
// second 32-row half of a tile is offset 4096, a stage 16384.
__device__ __forceinline__ void row_frag_addresses(uint32_t tile_lds, int lane, uint32_t (&a)[4])
{
    const int row = lane & 31, hi = lane >> 5;
#pragma unroll
    for (int t = 0; t < 4; ++t) a[t] = tile_lds + row * 128 + (((2 * t + hi) ^ tile_swz(row)) << 4);
}
#define LDS_READ128(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off))
#define ROW_FRAGS4(d, a, so, off)                                                                                   \
    do {                                                                                                            \
        LDS_READ128((d)[0], (a)[0] + (so), off); LDS_READ128((d)[1], (a)[1] + (so), off);                           \
        LDS_READ128((d)[2], (a)[2] + (so), off); LDS_READ128((d)[3], (a)[3] + (so), off);                           \
    } while (0)
#define LDS_WAIT4(d) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"((d)[0]), "+v"((d)[1]), "+v"((d)[2]), "+v"((d)[3])::"memory")
#define LDS_WAIT8(d, e)                                                                                             \
    asm volatile("s_waitcnt lgkmcnt(0)"                                                                             \
                 : "+v"((d)[0]), "+v"((d)[1]), "+v"((d)[2]), "+v"((d)[3]), "+v"((e)[0]), "+v"((e)[1]), "+v"((e)[2]), "+v"((e)[3])::"memory")

// Transposed fragments: for the 16-row k-step starting at tile row `rb` (multiple of 16) the lane (col c = jsub*32 + lane&31, half hi) gets rows
// rb + 4 hi + {0,1,2,3} and rb + 8 + 4 hi + {0,1,2,3} of column c -- the row subset a lane's accumulator registers 8(u&1)..8(u&1)+7 cover.
// tr_base[jsub][which] holds the lane's byte address for rb = 0.
__device__ __forceinline__ void tr_addresses(uint32_t tile_lds, int lane, uint32_t (&base)[2][2])
{
    const int t = lane & 15, colgrp = (lane >> 4) & 1, hi = lane >> 5;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = j * 32 + colgrp * 16 + (t & 3) * 4;
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            const int row = 4 * hi + 8 * w + (t >> 2);
            base[j][w] = tile_lds + row * 128 + ((((col >> 3) ^ tile_swz(row))) << 4) + (col & 7) * 2;
        }
    }
}
// k-step u = 0..3 covers tile rows 16 u .. 16 u + 15: tile_swz(row + 16 u) == tile_swz(row) ^ ... only bits (row>>1)&1 and (row>>2)&3 enter, and
// 16 u changes neither, so the address moves by the plain 2048-byte offset.
#define TR_FRAG(dst, base, u)                                                              \
    do {                                                                                   \
        uint2 lo_, hi_;                                                                    \
        TR_READ(lo_, (base)[0], (u) * 2048);                                               \
        TR_READ(hi_, (base)[1], (u) * 2048);                                               \
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(lo_), "+v"(hi_)::"memory");             \
        dst = __builtin_bit_cast(bf16x8, make_uint4(lo_.x, lo_.y, hi_.x, hi_.y));          \
    } while (0)

// Two / four transposed fragments with ONE wait: all reads go out first (they are independent), so their LDS latencies overlap
#define TR_FRAG2(d0, b0, d1, b1, u)                                                                                  \
    do {                                                                                                             \
        uint2 l0_, h0_, l1_, h1_;                                                                                    \
        TR_READ(l0_, (b0)[0], (u) * 2048); TR_READ(h0_, (b0)[1], (u) * 2048);                                        \
        TR_READ(l1_, (b1)[0], (u) * 2048); TR_READ(h1_, (b1)[1], (u) * 2048);                                        \
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(l0_), "+v"(h0_), "+v"(l1_), "+v"(h1_)::"memory");                 \
        d0 = __builtin_bit_cast(bf16x8, make_uint4(l0_.x, l0_.y, h0_.x, h0_.y));                                     \
        d1 = __builtin_bit_cast(bf16x8, make_uint4(l1_.x, l1_.y, h1_.x, h1_.y));                                     \
    } while (0)
#define TR_FRAG4(d0, b0, d1, b1, d2, b2, d3, b3, u)                                                                  \
    do {                                                                                                             \
        uint2 l0_, h0_, l1_, h1_, l2_, h2_, l3_, h3_;                                                                \
        TR_READ(l0_, (b0)[0], (u) * 2048); TR_READ(h0_, (b0)[1], (u) * 2048);                                        \
        TR_READ(l1_, (b1)[0], (u) * 2048); TR_READ(h1_, (b1)[1], (u) * 2048);                                        \
        TR_READ(l2_, (b2)[0], (u) * 2048); TR_READ(h2_, (b2)[1], (u) * 2048);                                        \
        TR_READ(l3_, (b3)[0], (u) * 2048); TR_READ(h3_, (b3)[1], (u) * 2048);                                        \
        asm volatile("s_waitcnt lgkmcnt(0)"                                                                          \
                     : "+v"(l0_), "+v"(h0_), "+v"(l1_), "+v"(h1_), "+v"(l2_), "+v"(h2_), "+v"(l3_), "+v"(h3_)::"memory"); \
        d0 = __builtin_bit_cast(bf16x8, make_uint4(l0_.x, l0_.y, h0_.x, h0_.y));                                     \
        d1 = __builtin_bit_cast(bf16x8, make_uint4(l1_.x, l1_.y, h1_.x, h1_.y));                                     \
        d2 = __builtin_bit_cast(bf16x8, make_uint4(l2_.x, l2_.y, h2_.x, h2_.y));                                     \
        d3 = __builtin_bit_cast(bf16x8, make_uint4(l3_.x, l3_.y, h3_.x, h3_.y));                                     \
    } while (0)

// 1-D grid decode shared by the attention kernels: workgroup ids go round-robin to the 8 XCDs (one L2 each); the blocks of one (batch,
// head) -- which stream the same K/V (or Q/dO) rows -- are given ids 8 apart so they land on the SAME XCD and the shared operand leaves HBM
// once.  With >= 64 sequences the HEADS of a sequence stay on one XCD as well (sequence b -> XCD b % 8, its heads and blocks consecutive
// there): a token's q / k / v for all heads are one contiguous row of the packed projection output, and short (packed) sequences are
// memory-bound -- 70 flop per byte at 140 tokens -- so it matters that the 128-byte head slices of a row are fetched by one L2 close
// together in time instead of by eight L2s at eight different moments.  Returns false for the padded tail.
__device__ __forceinline__ bool attn_decode(int id, int nblk, int total_bn, int heads, int &blk, int &b, int &n)
{
    const int xcd = id & 7, rest = id >> 3;
    blk = rest % nblk;
    const int r2 = rest / nblk;
    const int batch = total_bn / heads;
    if (batch >= 64) {
        n = r2 % heads;
        b = (r2 / heads) * 8 + xcd;
        return b < batch;
    }
    const int bn = r2 * 8 + xcd;
    if (bn >= total_bn) return false;
    b = bn / heads; n = bn - b * heads;
    return true;
}
__host__ __forceinline__ unsigned attn_grid(int nblk, int total_bn, int heads)
{
    const int batch = total_bn / heads;
    if (batch >= 64) return (unsigned)(((batch + 7) / 8) * 8 * heads * nblk);
    return (unsigned)(((total_bn + 7) / 8) * 8 * nblk);
}

// ---- one description of an attention launch's operands: what the forward's AttnParams and the backward's BwdParams both start with --------
#define KB 64              // keys per staged block
#define KSPLIT_BLOCKS 32   // key blocks (2,048 keys) per workgroup of a split-key launch: a sequence's ranges depend on ITS key count only
#define QBLOCK 128         // queries per workgroup of the forward and the dq kernel (four waves of 32)
struct AttnOperands {
    const char *q, *k, *v;
    const long long *ids_q, *ids_k;
    long long q_sb, q_ss, q_sn;   // element strides of q: batch, sequence, head
    long long k_sb, k_ss, k_sn, v_sb, v_ss, v_sn;
    int heads, sq, sk, causal, batch;
    float scale, drop_p;
    uint32_t seed;
    // packed ("varlen") operands: sequence b owns rows [cu[b], cu[b+1]) of a [rows, heads, 64] tensor (no batch stride, no padding rows);
    // NULL = the dense [batch, s] layout.  With cu_q the row statistics are laid out [heads, tq]; sq / sk are then the LONGEST sequence.
    const int *cu_q, *cu_k;
    long long tq;
    // split keys (few queries, very many keys: the FiD decoder's 32 positions over the ~20,000 packed keys of a question's K passages, where
    // one workgroup per (question, head) leaves most of the chip idle): the key blocks of a (batch, head, query block) are dealt to `ksplit`
    // workgroups, each leaves a partial in the launcher's workspace and a combine kernel folds them.  ksplit == 1: none of this.
    int ksplit;
    unsigned base_grid;           // workgroups of one split (attn_grid)
    long long stat_n;             // rows of the statistics: batch * heads * sq (dense) or heads * total_q (packed)
};

// this sequence's extent and operand offsets: dense = [b * s, b * s + s) with a batch stride; packed = rows [cu[b], cu[b+1])
struct SeqExtent {
    int sq, sk;
    long long qrow0, krow0, q_off, k_off, v_off, stat0;      // first row of the sequence in ids / o (q, k); element offsets; first statistic
};
__device__ __forceinline__ SeqExtent seq_extent(const AttnOperands &p, int b, int n)
{
    SeqExtent e;
    e.sq = p.sq; e.sk = p.sk;
    e.qrow0 = (long long)b * p.sq; e.krow0 = (long long)b * p.sk;
    e.q_off = (long long)b * p.q_sb; e.k_off = (long long)b * p.k_sb; e.v_off = (long long)b * p.v_sb;
    e.stat0 = ((long long)b * p.heads + n) * p.sq;
    if (p.cu_q) { const int c0 = p.cu_q[b]; e.sq = p.cu_q[b + 1] - c0; e.qrow0 = c0; e.q_off = (long long)c0 * p.q_ss; e.stat0 = (long long)n * p.tq + c0; }
    if (p.cu_k) { const int c0 = p.cu_k[b]; e.sk = p.cu_k[b + 1] - c0; e.krow0 = c0; e.k_off = (long long)c0 * p.k_ss; e.v_off = (long long)c0 * p.v_ss; }
    return e;
}

// Split keys: the number of key ranges of `sk` keys, and whether (and how many ways) a launch splits: ONE query block (<= 128 dense queries)
// over sequences of 4,096 keys or more.  A function of the launch's query / key EXTENTS only, never of the batch: the same question gives the
// same bits whether it runs alone, in a group of 8 or in a batch of 64 (question micro-batching relies on it), and short-key launches -- every
// shape the bf16-faithful oracle walks step by step -- never split.
__host__ __device__ __forceinline__ int attn_key_ranges(int sk) { return ((sk + KB - 1) / KB + KSPLIT_BLOCKS - 1) / KSPLIT_BLOCKS; }   // <= 32 (sk <= 65,536)
__host__ __forceinline__ int attention_ksplit(int max_sq, int max_sk) { return (max_sq > QBLOCK || max_sk < 4096) ? 1 : attn_key_ranges(max_sk); }
// a workgroup's key blocks [blk_lo, nblk): all of them, or its share of a split launch (possibly none: more splits than blocks)
__device__ __forceinline__ void split_block_range(int ksplit, int split, int sk, int &blk_lo, int &nblk)
{
    const int nblk_all = (sk + KB - 1) / KB;
    blk_lo = ksplit > 1 ? min(split * KSPLIT_BLOCKS, nblk_all) : 0;
    nblk = ksplit > 1 ? min((split + 1) * KSPLIT_BLOCKS, nblk_all) : nblk_all;
}

// LDS-DMA of one 64-key block into a 16 KiB stage (K tile, then V tile): 16 pieces of 1 KiB, wave w moves pieces w, w + WAVES, .. of each: 8 rows
// x 128 B, lane -> (row = 8 piece + lane>>3, LDS granule = lane&7), source granule = granule ^ tile_swz(row) (tile_swz looks at row bits 1..3:
// period 16, and a wave's pieces are 32 rows apart).  k_src / v_src: the sequence's first row of this head + the lane's source granule; prow =
// 8 wave + lane>>3.  dense: sk % 32 == 0 (checked on the host); packed: any sk.
template <int WAVES>
__device__ __forceinline__ void stage_kv_block(char *sb, const char *k_src, const char *v_src, long long k_ss, long long v_ss, int blk, int sk, int wave, int prow)
{
#pragma unroll
    for (int i = 0; i < 8 / WAVES; ++i) {
        long long key = blk * KB + prow + 8 * WAVES * i;
        if (key >= sk) key = sk - 1;                                           // keys past sk: re-read the last row, masked through its kmask bit (0)
        __builtin_amdgcn_global_load_lds((gptr_t *)(k_src + key * k_ss * 2), (lptr_t *)(sb + (wave + WAVES * i) * 1024), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((gptr_t *)(v_src + key * v_ss * 2), (lptr_t *)(sb + 8192 + (wave + WAVES * i) * 1024), 16, 0, 0);
    }
}
// key-padding bits of the blocks [blk_lo, nblk), one 64-bit word per block (bit = a real token inside the sequence)
template <int WAVES>
__device__ __forceinline__ void build_key_masks(unsigned long long *kmask_s, const long long *ids_k, long long krow0, int sk, int blk_lo, int nblk, int wave, int lane)
{
    for (int blk = blk_lo + wave; blk < nblk; blk += WAVES) {
        const int key = blk * KB + lane;
        const unsigned long long w = __builtin_amdgcn_ballot_w64(key < sk && ids_k[krow0 + (key < sk ? key : sk - 1)] != 0);
        if (lane == 0) kmask_s[blk] = w;
    }
}
// Epilogues: a lane holds d = j*32 + (r&3) + 8(r>>2) + 4*half of its row in acc[j][r].  The row as bf16 scaled by `s`, or as an fp32 partial.
__device__ __forceinline__ void store_row_bf16(uint16_t *row, const floatx16 (&acc)[2], float s, int hi)
{
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *(uint2 *)(row + j * 32 + 8 * g + 4 * hi) = make_uint2(pack_bf16(acc[j][4 * g] * s, acc[j][4 * g + 1] * s), pack_bf16(acc[j][4 * g + 2] * s, acc[j][4 * g + 3] * s));
}
__device__ __forceinline__ void store_row_partial(float *row, const floatx16 (&acc)[2], int hi)
{
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *(float4 *)(row + j * 32 + 8 * g + 4 * hi) = make_float4(acc[j][4 * g], acc[j][4 * g + 1], acc[j][4 * g + 2], acc[j][4 * g + 3]);
}

// ---- host side: the arguments both launchers take (the extern "C" entries of include/emdr2_ops.h fill them), each rule written once ---------
struct AttnArgs {
    const void *q; int64_t q_sb, q_ss, q_sn;                                   // the order of the entries' own arguments: they brace-initialise this
    const void *k; int64_t k_sb, k_ss, k_sn;
    const void *v; int64_t v_sb, v_ss, v_sn;
    const int64_t *ids_q, *ids_k;
    int batch, heads, sq, sk, head_dim, causal;                                // sq / sk: the longest sequence of a packed side
    float scale, drop_p; uint32_t seed; void *stream;
    const int32_t *cu_q = nullptr, *cu_k = nullptr; int64_t total_q = 0;       // packed sides
    double pairs = 0;                                                          // (query, key) pairs, for the op timer
    int ksplit = 1; void *ws = nullptr; size_t ws_bytes = 0;                   // split keys
    // The checks, in the order the launchers apply them (the order decides which code a doubly-wrong call gets):
    bool required() const { return q && k && v && ids_q && ids_k && batch >= 1 && heads >= 1 && sq >= 1; }                          // else -1
    bool split_args(bool policy) const { return ksplit >= 1 && ksplit <= 64 && (ksplit == 1 || (!cu_q && ws && !((uintptr_t)ws & 15) && policy)); }   // else -1
    bool shape_ok() const { return head_dim == 64 && sk >= 1 && sk <= 65536 && (cu_k || (sk >= 32 && !(sk & 31))); }   // else -4 (dense keys: whole 32-key steps)
    bool strides_ok() const { return !((q_sb | q_ss | q_sn | k_sb | k_ss | k_sn | v_sb | v_ss | v_sn) & 7); }                     // else -4
    bool packed_ok() const { return !cu_q || total_q >= 1; }                                                                       // else -1
    bool inputs_ok() const { return !(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15) && drop_p >= 0.f && drop_p < 1.f; }       // else -1
    void fill(AttnOperands &p) const
    {
        p.q = (const char *)q; p.k = (const char *)k; p.v = (const char *)v; p.ids_q = (const long long *)ids_q; p.ids_k = (const long long *)ids_k;
        p.q_sb = q_sb; p.q_ss = q_ss; p.q_sn = q_sn; p.k_sb = k_sb; p.k_ss = k_ss; p.k_sn = k_sn; p.v_sb = v_sb; p.v_ss = v_ss; p.v_sn = v_sn;
        p.heads = heads; p.sq = sq; p.sk = sk; p.causal = causal; p.scale = scale; p.drop_p = drop_p; p.seed = seed;
        p.batch = batch; p.cu_q = cu_q; p.cu_k = cu_k; p.tq = total_q;
        p.ksplit = ksplit; p.base_grid = attn_grid((sq + QBLOCK - 1) / QBLOCK, batch * heads, heads);
        p.stat_n = cu_q ? (long long)heads * total_q : (long long)batch * heads * sq;
    }
};
// the kernel instance for (dropout, history mask): f(std::bool_constant<DROP>, std::bool_constant<CAUSAL>)
template <class F>
static void attn_instance(bool drop, bool causal, F f)
{
    if (drop && causal) f(std::true_type{}, std::true_type{});
    else if (drop) f(std::true_type{}, std::false_type{});
    else if (causal) f(std::false_type{}, std::true_type{});
    else f(std::false_type{}, std::false_type{});
}
#endif
