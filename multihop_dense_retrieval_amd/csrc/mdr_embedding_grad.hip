// csrc/mdr_embedding_grad.hip -- the backward of the retriever's embedding layer on packed rows (include/mdr_embedding_grad.h): the plan
// (a stable sort of the tokens by table row, built once per forward), the segmented sum of d rows into the word and position tables, and
// the LayerNorm backward fused with the gather in front of it. The forward is embed_ln_kernel of csrc/mdr_encoder_pack_ln.inl,
//     x = (word[clamp(id)] + pos[min(pid, max_pos - 1)]) + type0,   y = (x - mu) * rstd * g + b,
// and it saves nothing: the backward recomputes x, mu and rstd from the tables.
//
// emb_keys_kernel: one thread per token t < total: its clamped word row and position row (the forward's clamps); writes the plan's header.
// emb_rank_kernel: rank by counting. A workgroup of four waves owns 64 tokens of one table, one per lane in every wave. The keys of all
//   tokens pass through LDS in tiles of 4096; wave w counts, over quarter w of each tile, the t' whose (row, t') is smaller than the lane's
//   (row, t): row' < row + (t' < t). Where a quarter lies wholly in front of or behind the workgroup's tokens the bound is hoisted.
//   The four counts are added through LDS and order[rank] = t. No data-dependent control flow, stable by construction.
// emb_segments_kernel: one workgroup per table walks the sorted tokens 1024 at a time, marks the heads (the row differs from the
//   predecessor's), numbers them by a ballot scan with a carry, and writes seg_start, seg_row and the number of segments.
// emb_scatter_kernel: a workgroup of eight waves owns a segment (a grid-stride loop over the segments of one table). A wave owns a piece
//   of P tokens: lane l holds columns l + 64 i and adds the piece's d rows from 0 in token order. The pieces go through LDS eight at a
//   time and thread e adds them from 0 in ascending piece order. The old value enters last. accumulate = 0: the table is zeroed on the stream first, then the same kernel writes the rows that own a segment.
// emb_ln_grad_kernel: the rows are cut into S chunks (grad_row_chunks: a function of (cap, H) alone); one workgroup of four waves owns a chunk,
//   a wave a token, with the forward's columns l + 64 i at every H. Wave w walks tokens w, w + 4, ... of the chunk in order, writes d of
//   each and keeps its lanes' dg, db and dtype0 columns in registers; the four waves' columns are added through LDS in wave order and go
//   to the workspace [S][3][H]. emb_colsum_kernel does the same for dtype0 alone from a given d ([S][1][H]): mdr_embedding_scatter.
// grad_strand_reduce_kernel (csrc/mdr_layernorm_grad.hip, through launch_strand_reduce of csrc/mdr_grad_common.h): strand j of sixteen adds
//   chunks j, j + 16, ... in order, the min(S, 16) strands are added in order, then the old value.
// Every output element has one owner and one summation order: no floating-point atomics, two runs give the same bits.
//
// Rounding points (tests/embedding_grad_ref.py derives its bound from this list; every operation is fp32, and a multiply feeding an add
// may be fused or not):
//   1. x = (w + p) + t0: two rounded adds. The forward's expression.
//   2. mu = wave_sum(s) / H: s adds the lane's H / 64 elements in index order, wave_sum is the xor butterfly 32, 16, .. 1; var the same
//      over (x - mu)^2; rstd = rsqrtf(var / H + eps). The forward's expressions in the forward's order.
//   3. dy = fp32(dy16) + fp32(dy2): one rounded add, none when only one is given.
//   4. xhat = (x - mu) * rstd, a = dy * g: one rounding each.
//   5. c1 = wave_sum(sum of a) / H and c2 = wave_sum(sum of a * xhat) / H: every term passes through at most H / 64 + 6 additions.
//   6. d = rstd * ((a - c1) - xhat * c2): not rounded again; the workspace holds it in fp32. dtype0 adds THAT value (the add is never fused with
//      the product), so that it has the bits of emb_colsum_kernel over the stored d.
//   7. A table row: the pieces' sums (at most P - 1 roundings: the first add is to 0), the pieces in order (at most ceil(n / P) - 1
//      roundings), the old value (one): at most P - 1 + ceil(n / P) + 1 additions per term.
//   8. dg += dy * xhat, db += dy and dtype0 += d per token in the wave's order; ((w0 + w1) + w2) + w3 over the waves; the chunks strand
//      by strand, the strands in order; the old value last. At most rows_per_chunk / 4 + 4 + S + 1 additions per element.
// Non-finite values propagate by IEEE rules alone: nothing float is clamped, compared or used as an index.
//
// The reader's flavour (include/mdr_reader_embedding_grad.h; the forward is reader_embed_ln_kernel of csrc/mdr_reader.inl,
//     x = (word[clamp(id)] + pos[tok_src % L]) + type[clamp(types[tok_src], 0, TV - 1)]):
// emb_reader_keys_kernel: emb_keys_kernel with the position row tok_src % L; the header carries MDR_READER_EMBEDDING_PLAN_MAGIC, a pad row PER
//   TABLE (words 7 and 8; the position table's is -1 for ELECTRA: row 0 is every sequence's [CLS]) and L (word 9). emb_rank_kernel and
//   emb_segments_kernel serve both kinds; the segments kernel takes the position table's pad row from word 8 when the magic is the reader's.
//   At most L distinct position rows, row p owning one token of every sequence longer than p: long segments, summed in the pieces above.
// emb_scatter_kernel is told the plan kind it differentiates (magic, L): a plan of the other kind, or of another L, makes it do nothing.
// emb_reader_ln_grad_kernel: emb_ln_grad_kernel's chunks, wave walk and expressions (rounding points 1 - 6 with t0 replaced by the token's
//   type row; 8 for dg and db). The type gradient is one plane per type row, TV <= 4: a token adds its STORED d (never fused, as point 6 says
//   of dtype0) to the plane of its own row and to no other, in the wave's token order (the planes are kept in LDS, one set per wave; the
//   kernel is a template over H / 64, which keeps it out of register spills); per plane the four waves are added ((w0 + w1) + w2) + w3 into part_ty [S][TV][H]; one
//   grad_strand_reduce_kernel over rows of TV * H columns
//   adds the chunks strand by strand, then the old value. dtype[k] therefore has the chunk, wave and strand split of dtype0 (a function of
//   (cap, H) alone) over the tokens of type k: at most rows_per_chunk / 4 + 4 + S + 1 additions per element, fewer where other types own
//   tokens. dg and db go through part_gb [S][2][H] and the same reduce. Without types every token is type 0, and dtype[0] has dtype0's bits.
#include <algorithm>
#include <climits>

#include "mdr_grad_common.h"
#include "../../include/mdr_embedding_grad.h"
#include "../../include/mdr_reader_embedding_grad.h"

namespace mdr {
namespace {

typedef int eg_int4 __attribute__((ext_vector_type(4)));

constexpr int kEgMaxCap = 1 << 20;
constexpr int kEgMaxVocab = 1 << 20;
constexpr int kEgMaxPos = 1 << 16;
constexpr int kEgMaxH = kGradMaxH;
constexpr int kEgPerLane = kEgMaxH / 64;
constexpr int kEgWaves = 4;
constexpr int kEgThreads = 64 * kEgWaves;
constexpr int kEgPiece = MDR_EMBEDDING_PIECE;
constexpr int kEgHeader = MDR_EMBEDDING_PLAN_HEADER;
constexpr int kEgRankQuarter = 1024;                    // keys a wave counts over per tile
constexpr int kEgRankTile = kEgRankQuarter * kEgWaves;  // keys in LDS at a time
constexpr int kEgSegThreads = 1024;
constexpr int kEgScatterWaves = 8;                      // pieces of a segment summed side by side
constexpr int kEgScatterThreads = 64 * kEgScatterWaves;
constexpr int kEgScatterGrid = 1 << 16;                 // most workgroups of emb_scatter_kernel per table
constexpr int kEgPlanes = 3;                            // dg, db, dtype0: the partial sums are [S][3][H] (the scatter's [S][1][H] uses the same split)

// kHdrPadPos and kHdrL are the reader plan's (MDR_READER_EMBEDDING_PLAN_MAGIC); a retriever plan leaves words 8 .. 15 zero
enum { kHdrMagic = 0, kHdrTotal, kHdrSegWord, kHdrSegPos, kHdrCap, kHdrVocab, kHdrMaxPos, kHdrPadRow, kHdrPadPos, kHdrL };
constexpr int kEgMaxTypes = MDR_READER_EMBEDDING_MAX_TYPES;

__host__ __device__ inline int eg_table_stride(int cap) { return (3 * cap + 1 + 3) / 4 * 4; }
__host__ __device__ inline int eg_table_off(int cap, int tbl) { return kEgHeader + tbl * eg_table_stride(cap); }
__host__ __device__ inline int eg_keys_off(int cap, int tbl) { return kEgHeader + 2 * eg_table_stride(cap) + tbl * cap; }
inline size_t eg_plan_words(int cap) { return (size_t)kEgHeader + 2 * (size_t)eg_table_stride(cap) + 2 * (size_t)cap; }

bool eg_cap_ok(int cap) { return cap >= 1 && cap <= kEgMaxCap; }

__device__ __forceinline__ int eg_total(const int* __restrict__ total, int cap) { return min(max(*total, 0), cap); }

// ---- the plan ----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) emb_keys_kernel(const long long* __restrict__ ids, const int* __restrict__ tok_src, const int* __restrict__ tok_pid,
                                                       const int* __restrict__ total_dev, int cap, int vocab, int max_pos, int pad_row, int* __restrict__ plan) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int total = eg_total(total_dev, cap);
    if (t < kEgHeader) {
        int v = 0;
        if (t == kHdrMagic) v = MDR_EMBEDDING_PLAN_MAGIC;
        if (t == kHdrTotal) v = total;
        if (t == kHdrCap) v = cap;
        if (t == kHdrVocab) v = vocab;
        if (t == kHdrMaxPos) v = max_pos;
        if (t == kHdrPadRow) v = pad_row;
        if (t != kHdrSegWord && t != kHdrSegPos) plan[t] = v;  // (the segment counts are emb_segments_kernel's)
    }
    if (t >= total) return;
    long long id = ids[tok_src[t]];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    int pid = tok_pid[t];
    pid = pid >= max_pos ? max_pos - 1 : (pid < 0 ? 0 : pid);
    plan[eg_keys_off(cap, 0) + t] = (int)id;
    plan[eg_keys_off(cap, 1) + t] = pid;
}

// the reader's keys: the position row is tok_src % L (no tok_pid), and the header carries the plan kind's magic, a pad row per table and L
__global__ void __launch_bounds__(256) emb_reader_keys_kernel(const long long* __restrict__ ids, const int* __restrict__ tok_src, const int* __restrict__ total_dev,
                                                              int cap, int L, int vocab, int max_pos, int pad_word, int pad_pos, int* __restrict__ plan) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int total = eg_total(total_dev, cap);
    if (t < kEgHeader) {
        int v = 0;
        if (t == kHdrMagic) v = MDR_READER_EMBEDDING_PLAN_MAGIC;
        if (t == kHdrTotal) v = total;
        if (t == kHdrCap) v = cap;
        if (t == kHdrVocab) v = vocab;
        if (t == kHdrMaxPos) v = max_pos;
        if (t == kHdrPadRow) v = pad_word;
        if (t == kHdrPadPos) v = pad_pos;
        if (t == kHdrL) v = L;
        if (t != kHdrSegWord && t != kHdrSegPos) plan[t] = v;  // (the segment counts are emb_segments_kernel's)
    }
    if (t >= total) return;
    const int src = tok_src[t];
    long long id = ids[src];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    int p = src % L;  // < L <= max_pos (checked on the host); the clamp keeps a negative tok_src, which the forward does not allow, in bounds
    p = p < 0 ? 0 : p;
    plan[eg_keys_off(cap, 0) + t] = (int)id;
    plan[eg_keys_off(cap, 1) + t] = p;
}

__global__ void __launch_bounds__(kEgThreads) emb_rank_kernel(int* __restrict__ plan, int cap) {
    __shared__ __attribute__((aligned(16))) int tile[kEgRankTile];
    __shared__ int counts[kEgWaves][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tbl = blockIdx.y;
    const int total = plan[kHdrTotal];
    const int b0 = blockIdx.x * 64;
    if (b0 >= total) return;  // (uniform over the workgroup)
    const int* keys = plan + eg_keys_off(cap, tbl);
    const int t = b0 + lane;
    const int my = t < total ? keys[t] : 0;
    int cnt = 0;
    for (int base = 0; base < total; base += kEgRankTile) {
#pragma unroll
        for (int j = 0; j < kEgRankTile / kEgThreads; ++j) {
            const int idx = base + j * kEgThreads + tid;
            tile[j * kEgThreads + tid] = idx < total ? keys[idx] : INT_MAX;  // (INT_MAX is below no bound: bounds are at most 2^20)
        }
        __syncthreads();
        const int k0 = base + wave * kEgRankQuarter;
        if (k0 < total) {
            const eg_int4* q = (const eg_int4*)(tile + wave * kEgRankQuarter);
            if (k0 + kEgRankQuarter <= b0 || k0 >= b0 + 64) {  // every t' of the quarter on one side of every t of the workgroup
                const int bound = my + (k0 < b0 ? 1 : 0);
#pragma unroll 8
                for (int i = 0; i < kEgRankQuarter / 4; ++i) {
                    const eg_int4 v = q[i];
                    cnt += (v[0] < bound) + (v[1] < bound) + (v[2] < bound) + (v[3] < bound);
                }
            } else {
#pragma unroll 4
                for (int i = 0; i < kEgRankQuarter / 4; ++i) {
                    const eg_int4 v = q[i];
                    const int tt = k0 + 4 * i;
                    cnt += (v[0] < my + (tt < t)) + (v[1] < my + (tt + 1 < t)) + (v[2] < my + (tt + 2 < t)) + (v[3] < my + (tt + 3 < t));
                }
            }
        }
        __syncthreads();
    }
    counts[wave][lane] = cnt;
    __syncthreads();
    if (wave == 0 && t < total) {
        const int r = ((counts[0][lane] + counts[1][lane]) + counts[2][lane]) + counts[3][lane];
        plan[eg_table_off(cap, tbl) + r] = t;  // r < total: the number of smaller tokens
    }
}

__global__ void __launch_bounds__(kEgSegThreads) emb_segments_kernel(int* __restrict__ plan, int cap) {
    __shared__ int wsum[kEgSegThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, tbl = blockIdx.x;
    const int total = plan[kHdrTotal];
    // a retriever plan has one pad row for both tables; a reader plan one per table
    const int pad_row = tbl && plan[kHdrMagic] == MDR_READER_EMBEDDING_PLAN_MAGIC ? plan[kHdrPadPos] : plan[kHdrPadRow];
    const int* keys = plan + eg_keys_off(cap, tbl);
    int* order = plan + eg_table_off(cap, tbl);
    int* seg_start = order + cap;
    int* seg_row = order + 2 * cap + 1;
    const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    int carry = 0;  // segments in front of this round (every thread keeps the same value)
    for (int base = 0; base < total; base += kEgSegThreads) {
        const int i = base + tid;
        int k = -1;
        bool head = false;
        if (i < total) {
            k = keys[min((unsigned)order[i], (unsigned)(total - 1))];  // (order is a permutation of 0 .. total - 1; the clamps keep a broken one in bounds)
            head = i == 0 || keys[min((unsigned)order[i - 1], (unsigned)(total - 1))] != k;
        }
        const unsigned long long bm = __ballot(head);
        if (lane == 0) wsum[w] = __popcll(bm);
        __syncthreads();
        int off = carry, all = 0;
#pragma unroll
        for (int j = 0; j < kEgSegThreads / 64; ++j) {
            const int c = wsum[j];
            if (j < w) off += c;
            all += c;
        }
        if (head) {
            const int s = off + __popcll(bm & lt);
            seg_start[s] = i;
            seg_row[s] = k == pad_row ? -1 - k : k;
        }
        carry += all;
        __syncthreads();
    }
    if (tid == 0) {
        seg_start[carry] = total;
        plan[kHdrSegWord + tbl] = carry;
    }
}

// ---- the segmented sum ---------------------------------------------------------------------------------------------------------------
// the sum of the d rows of tokens ord[0 .. n), n <= P, from 0 in token order: the lane's columns lane + 64 i. The loads of four rows are issued
// before their adds (one row at a time left the wave waiting for memory once per token); the order of the adds is the tokens'.
__device__ __forceinline__ void eg_piece_sum(const float* __restrict__ d32, int cap, const int* __restrict__ ord, int n, int H, int nl, int lane, float* acc) {
#pragma unroll
    for (int i = 0; i < kEgPerLane; ++i) acc[i] = 0.f;
    const unsigned last = (unsigned)(cap - 1);  // (ord[j] < total <= cap; the clamp keeps a broken plan in bounds)
    int j = 0;
    for (; j + 4 <= n; j += 4) {
        const float* r0 = d32 + (size_t)min((unsigned)ord[j], last) * H + lane;
        const float* r1 = d32 + (size_t)min((unsigned)ord[j + 1], last) * H + lane;
        const float* r2 = d32 + (size_t)min((unsigned)ord[j + 2], last) * H + lane;
        const float* r3 = d32 + (size_t)min((unsigned)ord[j + 3], last) * H + lane;
        float v0[kEgPerLane], v1[kEgPerLane], v2[kEgPerLane], v3[kEgPerLane];
#pragma unroll
        for (int i = 0; i < kEgPerLane; ++i)
            if (i < nl) { v0[i] = r0[64 * i]; v1[i] = r1[64 * i]; v2[i] = r2[64 * i]; v3[i] = r3[64 * i]; }
#pragma unroll
        for (int i = 0; i < kEgPerLane; ++i)
            if (i < nl) { acc[i] += v0[i]; acc[i] += v1[i]; acc[i] += v2[i]; acc[i] += v3[i]; }
    }
    for (; j < n; ++j) {
        const float* r = d32 + (size_t)min((unsigned)ord[j], last) * H + lane;
#pragma unroll
        for (int i = 0; i < kEgPerLane; ++i)
            if (i < nl) acc[i] += r[64 * i];
    }
}

__global__ void __launch_bounds__(kEgScatterThreads)
emb_scatter_kernel(const float* __restrict__ d32, const int* __restrict__ plan, int magic, int L, int cap, int H, int vocab, int max_pos, float* dword, float* dpos,
                   int accumulate) {
    __shared__ float red[kEgScatterWaves][kEgMaxH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tbl = blockIdx.y;
    float* out = tbl ? dpos : dword;
    if (!out) return;  // (uniform over the workgroup, as is every branch below but those on `wave`, `lane` and `tid`)
    // (magic, L): the plan kind the caller differentiates -- a retriever plan holds 0 at kHdrL. A plan of the other kind does nothing.
    if (plan[kHdrMagic] != magic || plan[kHdrL] != L || plan[kHdrCap] != cap || plan[kHdrVocab] != vocab || plan[kHdrMaxPos] != max_pos) return;
    const int nseg = min(plan[kHdrSegWord + tbl], plan[kHdrTotal]);
    const int* order = plan + eg_table_off(cap, tbl);
    const int* seg_start = order + cap;
    const int* seg_row = order + 2 * cap + 1;
    const int nl = H >> 6, nrows = tbl ? max_pos : vocab;
    for (int s = blockIdx.x; s < nseg; s += gridDim.x) {
        const int row = seg_row[s];
        if (row < 0) continue;  // pad_row: no gradient
        const int a = seg_start[s], n = seg_start[s + 1] - a;
        if (row >= nrows || a < 0 || n < 1 || a + n > cap) continue;  // (never in a plan of mdr_embedding_plan)
        float* o = out + (size_t)row * H;
        const int pieces = (n + kEgPiece - 1) / kEgPiece;
        float tot[kEgMaxH / kEgScatterThreads];
#pragma unroll
        for (int c = 0; c < kEgMaxH / kEgScatterThreads; ++c) tot[c] = 0.f;
        for (int p0 = 0; p0 < pieces; p0 += kEgScatterWaves) {
            const int p = p0 + wave;
            if (p < pieces) {
                float acc[kEgPerLane];
                eg_piece_sum(d32, cap, order + a + p * kEgPiece, min(kEgPiece, n - p * kEgPiece), H, nl, lane, acc);
#pragma unroll
                for (int i = 0; i < kEgPerLane; ++i)
                    if (i < nl) red[wave][lane + 64 * i] = acc[i];
            }
            __syncthreads();
            const int np = min(kEgScatterWaves, pieces - p0);
#pragma unroll
            for (int c = 0; c < kEgMaxH / kEgScatterThreads; ++c) {
                const int e = tid + kEgScatterThreads * c;
                if (e < H)
                    for (int w = 0; w < np; ++w) tot[c] += red[w][e];
            }
            __syncthreads();
        }
#pragma unroll
        for (int c = 0; c < kEgMaxH / kEgScatterThreads; ++c) {
            const int e = tid + kEgScatterThreads * c;
            if (e < H) o[e] = accumulate ? tot[c] + o[e] : tot[c];
        }
    }
}

// ---- sums over all valid tokens --------------------------------------------------------------------------------------------------------
// the four waves' per-lane columns v[plane][i] (column lane + 64 i) -> part[chunk][NP][H], ((w0 + w1) + w2) + w3
template <int NP>
__device__ __forceinline__ void eg_store_partials(float (*red)[3][kEgMaxH], const float (*v)[kEgPerLane], int nl, int H, float* __restrict__ part) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int pl = 0; pl < NP; ++pl)
#pragma unroll
        for (int i = 0; i < kEgPerLane; ++i)
            if (i < nl) red[wave][pl][lane + 64 * i] = v[pl][i];
    __syncthreads();
#pragma unroll
    for (int pl = 0; pl < NP; ++pl)
        for (int e = tid; e < H; e += kEgThreads)
            part[((size_t)blockIdx.x * NP + pl) * H + e] = ((red[0][pl][e] + red[1][pl][e]) + red[2][pl][e]) + red[3][pl][e];
}

__global__ void __launch_bounds__(kEgThreads)
emb_ln_grad_kernel(const long long* __restrict__ ids, const int* __restrict__ tok_src, const int* __restrict__ tok_pid, const int* __restrict__ total_dev,
                   int cap, const float* __restrict__ word, const float* __restrict__ pos, const float* __restrict__ type0, const float* __restrict__ g, int H,
                   int vocab, int max_pos, float eps, const _Float16* __restrict__ dy16, const void* __restrict__ dy2, int dy2_f32, int rpc,
                   float* __restrict__ d32, float* __restrict__ part) {
    __shared__ float red[kEgWaves][3][kEgMaxH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nl = H >> 6;
    const int total = eg_total(total_dev, cap);
    const int r0 = blockIdx.x * rpc, r1 = min(r0 + rpc, total);

    float gv[kEgPerLane], tv[kEgPerLane], sums[3][kEgPerLane];  // sums: dg, db, dtype0
#pragma unroll
    for (int i = 0; i < kEgPerLane; ++i) {
        if (i < nl) { gv[i] = g[lane + 64 * i]; tv[i] = type0[lane + 64 * i]; }
        sums[0][i] = sums[1][i] = sums[2][i] = 0.f;
    }
    for (int t = r0 + wave; t < r1; t += kEgWaves) {
        long long id = ids[tok_src[t]];
        id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
        int pid = tok_pid[t];
        pid = pid >= max_pos ? max_pos - 1 : (pid < 0 ? 0 : pid);
        const float* wr = word + (size_t)id * H;
        const float* pr = pos + (size_t)pid * H;
        const size_t off = (size_t)t * H;
        float x[kEgPerLane], dy[kEgPerLane];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < kEgPerLane; ++i)
            if (i < nl) {
                const int e = lane + 64 * i;
                x[i] = wr[e] + pr[e] + tv[i];
                s += x[i];
                if (dy16) {
                    dy[i] = (float)dy16[off + e];
                    if (dy2) dy[i] += dy2_f32 ? ((const float*)dy2)[off + e] : (float)((const _Float16*)dy2)[off + e];
                } else {
                    dy[i] = dy2_f32 ? ((const float*)dy2)[off + e] : (float)((const _Float16*)dy2)[off + e];
                }
            }
        const float mu = grad_wave_sum(s) / H;
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < kEgPerLane; ++i)
            if (i < nl) { const float dlt = x[i] - mu; v += dlt * dlt; }
        const float rstd = rsqrtf(grad_wave_sum(v) / H + eps);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < kEgPerLane; ++i)
            if (i < nl) {
                const float xh = (x[i] - mu) * rstd;
                const float a = dy[i] * gv[i];
                s1 += a;
                s2 += a * xh;
                sums[0][i] += dy[i] * xh;
                sums[1][i] += dy[i];
                x[i] = xh;
                dy[i] = a;
            }
        const float c1 = grad_wave_sum(s1) / H, c2 = grad_wave_sum(s2) / H;
#pragma unroll
        for (int i = 0; i < kEgPerLane; ++i)
            if (i < nl) {
                const float d = rstd * ((dy[i] - c1) - x[i] * c2);
                {
                    // dtype0 adds the d that is STORED: fused into the product, the add took rstd * (..) unrounded, and from the second token
                    // of a wave on (rows_per_chunk > 4) dtype0 no longer had the bits of emb_colsum_kernel over the same d
#pragma clang fp contract(off)
                    sums[2][i] += d;
                }
                d32[off + lane + 64 * i] = d;
            }
    }
    if (part) eg_store_partials<3>(red, sums, nl, H, part);
}

__global__ void __launch_bounds__(kEgThreads)
emb_colsum_kernel(const float* __restrict__ d32, const int* __restrict__ plan, int cap, int H, int rpc, float* __restrict__ part) {
    __shared__ float red[kEgWaves][3][kEgMaxH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nl = H >> 6;
    const int total = plan[kHdrMagic] == MDR_EMBEDDING_PLAN_MAGIC && plan[kHdrCap] == cap ? min(max(plan[kHdrTotal], 0), cap) : 0;
    const int r0 = blockIdx.x * rpc, r1 = min(r0 + rpc, total);
    float sums[1][kEgPerLane];
#pragma unroll
    for (int i = 0; i < kEgPerLane; ++i) sums[0][i] = 0.f;
    for (int t = r0 + wave; t < r1; t += kEgWaves) {
        const float* r = d32 + (size_t)t * H + lane;
#pragma unroll
        for (int i = 0; i < kEgPerLane; ++i)
            if (i < nl) sums[0][i] += r[64 * i];
    }
    eg_store_partials<1>(red, sums, nl, H, part);
}

// The reader's flavour of emb_ln_grad_kernel (the forward is reader_embed_ln_kernel of csrc/mdr_reader.inl): the position row is tok_src % L, the
// type row clamp(types[tok_src], 0, TV - 1) of a [TV, H] table (row 0 without types). Same chunks, same wave walk, same d; the type gradient
// is one plane per type row: a token adds its d to the plane of its own row only. The planes live in LDS, one set per wave (a lane owns its
// columns lane + 64 i of its wave's planes, so the walk needs no barrier). NL = H / 64 is a template argument here: with the other flavour's
// sixteen `i < nl` tests and this one's longer argument list the scalar registers no longer sufficed. part_gb [S][2][H] (dg, db), part_ty [S][TV][H].
template <int NL>
__global__ void __launch_bounds__(kEgThreads)
emb_reader_ln_grad_kernel(const long long* __restrict__ ids, const long long* __restrict__ types, const int* __restrict__ tok_src, const int* __restrict__ total_dev,
                          int cap, int L, const float* __restrict__ word, const float* __restrict__ pos, const float* __restrict__ type_emb, int TV,
                          const float* __restrict__ g, int vocab, float eps, const _Float16* __restrict__ dy16, const void* __restrict__ dy2, int dy2_f32, int rpc,
                          float* __restrict__ d32, float* __restrict__ part_gb, float* __restrict__ part_ty) {
    constexpr int H = 64 * NL;
    __shared__ float ts[kEgWaves][kEgMaxTypes][H];  // dtype[k] of each wave; afterwards planes 0 and 1 carry the waves' dg and db
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int total = eg_total(total_dev, cap);
    const int r0 = blockIdx.x * rpc, r1 = min(r0 + rpc, total);

    float gv[NL], sums[2][NL];  // sums: dg, db
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        gv[i] = g[lane + 64 * i];
        sums[0][i] = sums[1][i] = 0.f;
    }
    for (int k = 0; k < TV; ++k)
#pragma unroll
        for (int i = 0; i < NL; ++i) ts[wave][k][lane + 64 * i] = 0.f;
    for (int t = r0 + wave; t < r1; t += kEgWaves) {
        const int src = tok_src[t];
        int p = src % L;
        p = p < 0 ? 0 : p;
        long long id = ids[src];
        id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
        long long tyl = types ? types[src] : 0;
        const int ty = (int)(tyl < 0 ? 0 : (tyl >= TV ? TV - 1 : tyl));  // (uniform over the wave)
        const float* wr = word + (size_t)id * H + lane;
        const float* pr = pos + (size_t)p * H + lane;
        const float* tr = type_emb + (size_t)ty * H + lane;
        float* tsr = &ts[wave][ty][lane];
        const size_t off = (size_t)t * H + lane;
        float x[NL], dy[NL];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int e = 64 * i;
            x[i] = wr[e] + pr[e] + tr[e];
            s += x[i];
            if (dy16) {
                dy[i] = (float)dy16[off + e];
                if (dy2) dy[i] += dy2_f32 ? ((const float*)dy2)[off + e] : (float)((const _Float16*)dy2)[off + e];
            } else {
                dy[i] = dy2_f32 ? ((const float*)dy2)[off + e] : (float)((const _Float16*)dy2)[off + e];
            }
        }
        const float mu = grad_wave_sum(s) / H;
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < NL; ++i) { const float dlt = x[i] - mu; v += dlt * dlt; }
        const float rstd = rsqrtf(grad_wave_sum(v) / H + eps);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const float xh = (x[i] - mu) * rstd;
            const float a = dy[i] * gv[i];
            s1 += a;
            s2 += a * xh;
            sums[0][i] += dy[i] * xh;
            sums[1][i] += dy[i];
            x[i] = xh;
            dy[i] = a;
        }
        const float c1 = grad_wave_sum(s1) / H, c2 = grad_wave_sum(s2) / H;
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const float d = rstd * ((dy[i] - c1) - x[i] * c2);
            {
                // dtype adds the d that is STORED, never fused with the product (emb_ln_grad_kernel's rule)
#pragma clang fp contract(off)
                tsr[64 * i] += d;
            }
            d32[off + 64 * i] = d;
        }
    }
    __syncthreads();
    if (part_ty)
        for (int k = 0; k < TV; ++k)
            for (int e = tid; e < H; e += kEgThreads)
                part_ty[((size_t)blockIdx.x * TV + k) * H + e] = ((ts[0][k][e] + ts[1][k][e]) + ts[2][k][e]) + ts[3][k][e];
    if (!part_gb) return;  // (uniform)
    __syncthreads();  // the type planes are read: planes 0 and 1 now carry dg and db, added as eg_store_partials adds them
#pragma unroll
    for (int pl = 0; pl < 2; ++pl)
#pragma unroll
        for (int i = 0; i < NL; ++i) ts[wave][pl][lane + 64 * i] = sums[pl][i];
    __syncthreads();
#pragma unroll
    for (int pl = 0; pl < 2; ++pl)
        for (int e = tid; e < H; e += kEgThreads)
            part_gb[((size_t)blockIdx.x * 2 + pl) * H + e] = ((ts[0][pl][e] + ts[1][pl][e]) + ts[2][pl][e]) + ts[3][pl][e];
}

// the table half of both entry points: accumulate = 0 zeroes the given tables first
int eg_launch_tables(const float* d32, const int* plan, int magic, int L, int cap, int H, int vocab, int max_pos, float* dword, float* dpos, int accumulate,
                     hipStream_t st) {
    if (!dword && !dpos) return MDR_OK;
    if (!accumulate) {
        if (dword) MDR_HIP_TRY(hipMemsetAsync(dword, 0, (size_t)vocab * H * sizeof(float), st));
        if (dpos) MDR_HIP_TRY(hipMemsetAsync(dpos, 0, (size_t)max_pos * H * sizeof(float), st));
    }
    hipLaunchKernelGGL(emb_scatter_kernel, dim3(std::min(cap, kEgScatterGrid), 2), dim3(kEgScatterThreads), 0, st, d32, plan, magic, L, cap, H,
                       vocab, max_pos, dword, dpos, accumulate);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

}  // namespace
}  // namespace mdr

extern "C" {

size_t mdr_embedding_plan_bytes(int cap) {
    using namespace mdr;
    return eg_cap_ok(cap) ? align_up(eg_plan_words(cap) * sizeof(int), 256) : 0;
}

int mdr_embedding_plan(const int64_t* ids_dev, const int* tok_src_dev, const int* tok_pid_dev, const int* total_dev, int cap, int vocab, int max_pos,
                       int pad_row, void* plan_dev, size_t plan_bytes, int device, void* stream) {
    using namespace mdr;
    const char* fn = "mdr_embedding_plan";
    MDR_REQUIRE(ids_dev && tok_src_dev && tok_pid_dev && total_dev, "%s: NULL pointer (ids, tok_src, tok_pid and total are required)", fn);
    MDR_REQUIRE(eg_cap_ok(cap), "%s: cap=%d out of range (1 .. 2^20)", fn, cap);
    MDR_REQUIRE(vocab >= 1 && vocab <= kEgMaxVocab, "%s: vocab=%d out of range (1 .. 2^20)", fn, vocab);
    MDR_REQUIRE(max_pos >= 1 && max_pos <= kEgMaxPos, "%s: max_pos=%d out of range (1 .. 2^16)", fn, max_pos);
    MDR_REQUIRE(pad_row >= -1 && pad_row < kEgMaxVocab, "%s: pad_row=%d out of range (-1 .. 2^20 - 1)", fn, pad_row);
    MDR_REQUIRE(aligned16({plan_dev}), "%s: the plan must be 16-byte aligned", fn);
    const size_t need = eg_plan_words(cap) * sizeof(int);
    if (!(plan_dev && plan_bytes >= need))
        return set_error(MDR_E_WORKSPACE, "%s: plan buffer of %zu bytes, need %zu (mdr_embedding_plan_bytes)", fn, plan_dev ? plan_bytes : (size_t)0, need);
    MDR_ENTER_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    int* plan = (int*)plan_dev;
    hipLaunchKernelGGL(emb_keys_kernel, dim3((std::max(cap, kEgHeader) + 255) / 256), dim3(256), 0, st, (const long long*)ids_dev, tok_src_dev, tok_pid_dev, total_dev,
                       cap, vocab, max_pos, pad_row, plan);
    MDR_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(emb_rank_kernel, dim3((cap + 63) / 64, 2), dim3(kEgThreads), 0, st, plan, cap);
    MDR_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(emb_segments_kernel, dim3(2), dim3(kEgSegThreads), 0, st, plan, cap);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

int mdr_embedding_backward_chunks(int cap, int H, int* rows_per_chunk) {
    using namespace mdr;
    int rpc = 0, S = 0;
    if (eg_cap_ok(cap) && grad_hidden_ok(H)) S = grad_row_chunks(cap, H, kEgPlanes, &rpc);
    if (rows_per_chunk) *rows_per_chunk = rpc;
    return S;
}

size_t mdr_embedding_scatter_workspace_bytes(int cap, int H) {
    using namespace mdr;
    if (!(eg_cap_ok(cap) && grad_hidden_ok(H))) return 0;
    int rpc;
    return align_up((size_t)grad_row_chunks(cap, H, kEgPlanes, &rpc) * H * sizeof(float), 256);
}

size_t mdr_embedding_backward_workspace_bytes(int cap, int H) {
    using namespace mdr;
    if (!(eg_cap_ok(cap) && grad_hidden_ok(H))) return 0;
    int rpc;
    return align_up((size_t)cap * H * sizeof(float), 256) + align_up((size_t)grad_row_chunks(cap, H, kEgPlanes, &rpc) * 3 * H * sizeof(float), 256);
}

int mdr_embedding_scatter(const float* d32_dev, const void* plan_dev, int cap, int H, int vocab, int max_pos, float* dword_dev, float* dpos_dev,
                          float* dtype0_dev, int accumulate, void* workspace_dev, size_t workspace_bytes, int device, void* stream) {
    using namespace mdr;
    const char* fn = "mdr_embedding_scatter";
    MDR_REQUIRE(d32_dev && plan_dev, "%s: NULL pointer (d32 and the plan are required)", fn);
    MDR_REQUIRE(dword_dev || dpos_dev || dtype0_dev, "%s: NULL pointer (every output: at least one is required)", fn);
    MDR_REQUIRE(accumulate == 0 || accumulate == 1, "%s: accumulate must be 0 or 1, got %d", fn, accumulate);
    MDR_REQUIRE(eg_cap_ok(cap), "%s: cap=%d out of range (1 .. 2^20)", fn, cap);
    MDR_REQUIRE(grad_hidden_ok(H), "%s: H=%d unsupported (a multiple of 64, 64 .. 1024)", fn, H);
    MDR_REQUIRE(vocab >= 1 && vocab <= kEgMaxVocab, "%s: vocab=%d out of range (1 .. 2^20)", fn, vocab);
    MDR_REQUIRE(max_pos >= 1 && max_pos <= kEgMaxPos, "%s: max_pos=%d out of range (1 .. 2^16)", fn, max_pos);
    MDR_REQUIRE(aligned16({d32_dev, plan_dev, dword_dev, dpos_dev, dtype0_dev, workspace_dev}), "%s: every pointer must be 16-byte aligned", fn);
    int rpc;
    const int S = grad_row_chunks(cap, H, kEgPlanes, &rpc);
    const size_t need = dtype0_dev ? (size_t)S * H * sizeof(float) : 0;
    MDR_REQUIRE_WORKSPACE(fn, workspace_dev, workspace_bytes, need, "mdr_embedding_scatter_workspace_bytes");
    MDR_ENTER_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    const int* plan = (const int*)plan_dev;
    if (dtype0_dev) {
        float* part = (float*)workspace_dev;
        hipLaunchKernelGGL(emb_colsum_kernel, dim3(S), dim3(kEgThreads), 0, st, d32_dev, plan, cap, H, rpc, part);
        MDR_HIP_TRY(hipGetLastError());
        if (int rc = launch_strand_reduce(part, S, 1, H, dtype0_dev, nullptr, nullptr, accumulate, st)) return rc;
    }
    return eg_launch_tables(d32_dev, plan, MDR_EMBEDDING_PLAN_MAGIC, 0, cap, H, vocab, max_pos, dword_dev, dpos_dev, accumulate, st);
}

int mdr_embedding_backward(const int64_t* ids_dev, const int* tok_src_dev, const int* tok_pid_dev, const int* total_dev, int cap, const float* word_dev,
                           const float* pos_dev, const float* type0_dev, const float* g_dev, int H, int vocab, int max_pos, float eps, const void* dy16_dev,
                           const void* dy2_dev, int dy2_f32, const void* plan_dev, float* dword_dev, float* dpos_dev, float* dtype0_dev, float* dg_dev,
                           float* db_dev, float* d32_dev, int accumulate, void* workspace_dev, size_t workspace_bytes, int device, void* stream) {
    using namespace mdr;
    const char* fn = "mdr_embedding_backward";
    MDR_REQUIRE(ids_dev && tok_src_dev && tok_pid_dev && total_dev, "%s: NULL pointer (ids, tok_src, tok_pid and total are required)", fn);
    MDR_REQUIRE(word_dev && pos_dev && type0_dev && g_dev, "%s: NULL pointer (word, pos, type0 and g are required)", fn);
    MDR_REQUIRE(dy16_dev || dy2_dev, "%s: NULL pointer (dy16 and dy2: at least one is required)", fn);
    MDR_REQUIRE(dword_dev || dpos_dev || dtype0_dev || dg_dev || db_dev || d32_dev, "%s: NULL pointer (every output: at least one is required)", fn);
    MDR_REQUIRE(plan_dev || !(dword_dev || dpos_dev), "%s: NULL pointer (dword and dpos need the plan)", fn);
    MDR_REQUIRE(dy2_f32 == 0 || dy2_f32 == 1, "%s: dy2_f32 must be 0 or 1, got %d", fn, dy2_f32);
    MDR_REQUIRE(accumulate == 0 || accumulate == 1, "%s: accumulate must be 0 or 1, got %d", fn, accumulate);
    MDR_REQUIRE(eg_cap_ok(cap), "%s: cap=%d out of range (1 .. 2^20)", fn, cap);
    MDR_REQUIRE(grad_hidden_ok(H), "%s: H=%d unsupported (a multiple of 64, 64 .. 1024)", fn, H);
    MDR_REQUIRE(vocab >= 1 && vocab <= kEgMaxVocab, "%s: vocab=%d out of range (1 .. 2^20)", fn, vocab);
    MDR_REQUIRE(max_pos >= 1 && max_pos <= kEgMaxPos, "%s: max_pos=%d out of range (1 .. 2^16)", fn, max_pos);
    MDR_REQUIRE(aligned16({word_dev, pos_dev, type0_dev, g_dev, dy16_dev, dy2_dev, plan_dev, dword_dev, dpos_dev, dtype0_dev, dg_dev, db_dev, d32_dev,
                              workspace_dev}),
                "%s: every float, plan and workspace pointer must be 16-byte aligned", fn);
    int rpc;
    const int S = grad_row_chunks(cap, H, kEgPlanes, &rpc);
    const size_t d_bytes = align_up((size_t)cap * H * sizeof(float), 256);
    const size_t need = d_bytes + (size_t)S * 3 * H * sizeof(float);
    MDR_REQUIRE_WORKSPACE(fn, workspace_dev, workspace_bytes, need, "mdr_embedding_backward_workspace_bytes");
    MDR_ENTER_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    float* d32 = d32_dev ? d32_dev : (float*)workspace_dev;  // d goes where the caller wants to see it
    const bool sums = dtype0_dev || dg_dev || db_dev;
    float* part = sums ? (float*)((char*)workspace_dev + d_bytes) : nullptr;
    hipLaunchKernelGGL(emb_ln_grad_kernel, dim3(S), dim3(kEgThreads), 0, st, (const long long*)ids_dev, tok_src_dev, tok_pid_dev, total_dev, cap, word_dev, pos_dev,
                       type0_dev, g_dev, H, vocab, max_pos, eps, (const _Float16*)dy16_dev, dy2_dev, dy2_f32, rpc, d32, part);
    MDR_HIP_TRY(hipGetLastError());
    if (part)
        if (int rc = launch_strand_reduce(part, S, kEgPlanes, H, dg_dev, db_dev, dtype0_dev, accumulate, st)) return rc;
    return eg_launch_tables(d32, (const int*)plan_dev, MDR_EMBEDDING_PLAN_MAGIC, 0, cap, H, vocab, max_pos, dword_dev, dpos_dev, accumulate, st);
}

// ---- the reader's flavour (include/mdr_reader_embedding_grad.h) ------------------------------------------------------------------------
int mdr_reader_embedding_plan(const int64_t* ids_dev, const int* tok_src_dev, const int* total_dev, int cap, int L, int vocab, int max_pos, int pad_word,
                              int pad_pos, void* plan_dev, size_t plan_bytes, int device, void* stream) {
    using namespace mdr;
    const char* fn = "mdr_reader_embedding_plan";
    MDR_REQUIRE(ids_dev && tok_src_dev && total_dev, "%s: NULL pointer (ids, tok_src and total are required)", fn);
    MDR_REQUIRE(eg_cap_ok(cap), "%s: cap=%d out of range (1 .. 2^20)", fn, cap);
    MDR_REQUIRE(vocab >= 1 && vocab <= kEgMaxVocab, "%s: vocab=%d out of range (1 .. 2^20)", fn, vocab);
    MDR_REQUIRE(max_pos >= 1 && max_pos <= kEgMaxPos, "%s: max_pos=%d out of range (1 .. 2^16)", fn, max_pos);
    MDR_REQUIRE(L >= 1 && L <= max_pos, "%s: L=%d out of range (1 .. max_pos=%d)", fn, L, max_pos);
    MDR_REQUIRE(pad_word >= -1 && pad_word < kEgMaxVocab, "%s: pad_word=%d out of range (-1 .. 2^20 - 1)", fn, pad_word);
    MDR_REQUIRE(pad_pos >= -1 && pad_pos < kEgMaxPos, "%s: pad_pos=%d out of range (-1 .. 2^16 - 1)", fn, pad_pos);
    MDR_REQUIRE(aligned16({plan_dev}), "%s: the plan must be 16-byte aligned", fn);
    const size_t need = eg_plan_words(cap) * sizeof(int);
    if (!(plan_dev && plan_bytes >= need))
        return set_error(MDR_E_WORKSPACE, "%s: plan buffer of %zu bytes, need %zu (mdr_embedding_plan_bytes)", fn, plan_dev ? plan_bytes : (size_t)0, need);
    MDR_ENTER_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    int* plan = (int*)plan_dev;
    hipLaunchKernelGGL(emb_reader_keys_kernel, dim3((std::max(cap, kEgHeader) + 255) / 256), dim3(256), 0, st, (const long long*)ids_dev, tok_src_dev, total_dev, cap, L,
                       vocab, max_pos, pad_word, pad_pos, plan);
    MDR_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(emb_rank_kernel, dim3((cap + 63) / 64, 2), dim3(kEgThreads), 0, st, plan, cap);
    MDR_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(emb_segments_kernel, dim3(2), dim3(kEgSegThreads), 0, st, plan, cap);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

size_t mdr_reader_embedding_backward_workspace_bytes(int cap, int H, int type_vocab) {
    using namespace mdr;
    if (!(eg_cap_ok(cap) && grad_hidden_ok(H) && type_vocab >= 1 && type_vocab <= kEgMaxTypes)) return 0;
    int rpc;
    const size_t S = (size_t)grad_row_chunks(cap, H, kEgPlanes, &rpc);
    return align_up((size_t)cap * H * sizeof(float), 256) + align_up(S * 2 * H * sizeof(float), 256) + align_up(S * type_vocab * H * sizeof(float), 256);
}

int mdr_reader_embedding_backward(const int64_t* ids_dev, const int64_t* types_dev, const int* tok_src_dev, const int* total_dev, int cap, int L,
                                  const float* word_dev, const float* pos_dev, const float* type_dev, int type_vocab, const float* g_dev, int H, int vocab,
                                  int max_pos, float eps, const void* dy16_dev, const void* dy2_dev, int dy2_f32, const void* plan_dev, float* dword_dev,
                                  float* dpos_dev, float* dtype_dev, float* dg_dev, float* db_dev, float* d32_dev, int accumulate, void* workspace_dev,
                                  size_t workspace_bytes, int device, void* stream) {
    using namespace mdr;
    const char* fn = "mdr_reader_embedding_backward";
    MDR_REQUIRE(ids_dev && tok_src_dev && total_dev, "%s: NULL pointer (ids, tok_src and total are required; types may be NULL)", fn);
    MDR_REQUIRE(word_dev && pos_dev && type_dev && g_dev, "%s: NULL pointer (word, pos, type and g are required)", fn);
    MDR_REQUIRE(dy16_dev || dy2_dev, "%s: NULL pointer (dy16 and dy2: at least one is required)", fn);
    MDR_REQUIRE(dword_dev || dpos_dev || dtype_dev || dg_dev || db_dev || d32_dev, "%s: NULL pointer (every output: at least one is required)", fn);
    MDR_REQUIRE(plan_dev || !(dword_dev || dpos_dev), "%s: NULL pointer (dword and dpos need the plan)", fn);
    MDR_REQUIRE(dy2_f32 == 0 || dy2_f32 == 1, "%s: dy2_f32 must be 0 or 1, got %d", fn, dy2_f32);
    MDR_REQUIRE(accumulate == 0 || accumulate == 1, "%s: accumulate must be 0 or 1, got %d", fn, accumulate);
    MDR_REQUIRE(eg_cap_ok(cap), "%s: cap=%d out of range (1 .. 2^20)", fn, cap);
    MDR_REQUIRE(grad_hidden_ok(H), "%s: H=%d unsupported (a multiple of 64, 64 .. 1024)", fn, H);
    MDR_REQUIRE(vocab >= 1 && vocab <= kEgMaxVocab, "%s: vocab=%d out of range (1 .. 2^20)", fn, vocab);
    MDR_REQUIRE(max_pos >= 1 && max_pos <= kEgMaxPos, "%s: max_pos=%d out of range (1 .. 2^16)", fn, max_pos);
    MDR_REQUIRE(L >= 1 && L <= max_pos, "%s: L=%d out of range (1 .. max_pos=%d)", fn, L, max_pos);
    MDR_REQUIRE(type_vocab >= 1 && type_vocab <= kEgMaxTypes, "%s: type_vocab=%d out of range (1 .. %d)", fn, type_vocab, kEgMaxTypes);
    MDR_REQUIRE(aligned16({word_dev, pos_dev, type_dev, g_dev, dy16_dev, dy2_dev, plan_dev, dword_dev, dpos_dev, dtype_dev, dg_dev, db_dev, d32_dev,
                              workspace_dev}),
                "%s: every float, plan and workspace pointer must be 16-byte aligned", fn);
    int rpc;
    const int S = grad_row_chunks(cap, H, kEgPlanes, &rpc);  // the split of mdr_embedding_backward_chunks: a function of (cap, H) alone
    const size_t d_bytes = align_up((size_t)cap * H * sizeof(float), 256);
    const size_t gb_bytes = align_up((size_t)S * 2 * H * sizeof(float), 256);
    const size_t need = d_bytes + gb_bytes + (size_t)S * type_vocab * H * sizeof(float);
    MDR_REQUIRE_WORKSPACE(fn, workspace_dev, workspace_bytes, need, "mdr_reader_embedding_backward_workspace_bytes");
    MDR_ENTER_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    float* d32 = d32_dev ? d32_dev : (float*)workspace_dev;
    float* part_gb = dg_dev || db_dev ? (float*)((char*)workspace_dev + d_bytes) : nullptr;
    float* part_ty = dtype_dev ? (float*)((char*)workspace_dev + d_bytes + gb_bytes) : nullptr;
#define MDR_EG_READER(NL)                                                                                                                                          \
    case NL:                                                                                                                                                       \
        hipLaunchKernelGGL(emb_reader_ln_grad_kernel<NL>, dim3(S), dim3(kEgThreads), 0, st, (const long long*)ids_dev, (const long long*)types_dev, tok_src_dev,  \
                           total_dev, cap, L, word_dev, pos_dev, type_dev, type_vocab, g_dev, vocab, eps, (const _Float16*)dy16_dev, dy2_dev, dy2_f32, rpc, d32,   \
                           part_gb, part_ty);                                                                                                                      \
        break;
    switch (H >> 6) {  // (1 .. 16: grad_hidden_ok)
        MDR_EG_READER(1) MDR_EG_READER(2) MDR_EG_READER(3) MDR_EG_READER(4) MDR_EG_READER(5) MDR_EG_READER(6) MDR_EG_READER(7) MDR_EG_READER(8)
        MDR_EG_READER(9) MDR_EG_READER(10) MDR_EG_READER(11) MDR_EG_READER(12) MDR_EG_READER(13) MDR_EG_READER(14) MDR_EG_READER(15) MDR_EG_READER(16)
    }
#undef MDR_EG_READER
    MDR_HIP_TRY(hipGetLastError());
    if (part_gb)
        if (int rc = launch_strand_reduce(part_gb, S, 2, H, dg_dev, db_dev, nullptr, accumulate, st)) return rc;
    // the type table's planes are [S][type_vocab * H]: one strand reduce over rows of type_vocab * H columns writes dtype [type_vocab, H]
    if (part_ty)
        if (int rc = launch_strand_reduce(part_ty, S, 1, type_vocab * H, dtype_dev, nullptr, nullptr, accumulate, st)) return rc;
    return eg_launch_tables(d32, (const int*)plan_dev, MDR_READER_EMBEDDING_PLAN_MAGIC, L, cap, H, vocab, max_pos, dword_dev, dpos_dev, accumulate, st);
}

}  // extern "C"
