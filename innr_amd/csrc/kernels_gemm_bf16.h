// kernels_gemm_bf16.h -- the GEMM engine's FILTER on the bf16 pipe (v_mfma_f32_32x32x16_bf16, 16x the f32 MFMA rate).
//
// Same contract as gemm_filter_kernel (kernels_gemm.h): approximate scores in, per-(slice, query) candidate lists out;
// the caller re-scores the candidates in the reference's f32 order and proves the answer, so the results stay the
// reference's bit for bit (batch.rs:742-764) -- only the approximation bound E changes: both operands are rounded to
// bf16 (relative 2^-9 each), so |score_bf16 - score| <= (2^-8 + 2^-16) sum|q_d v_d| + the f32 accumulation term.
//
// Layouts (built once per corpus / once per call by the pack kernels below):
//   corpus  Ab[tile][ks][kg 0..3][rt 0..3][i 0..31][8 bf16]   corpus row = 128 tile + 4 i + rt, dimension = 32 ks + 8 kg + e
//           one K-step (32 dimensions) of a 128-row tile is 8 KiB contiguous: eight 1-KiB LDS-DMA pieces, one per wave;
//           an A fragment (row i of row tile rt, 8 consecutive k) is one conflict-free ds_read_b128.
//   queries Bb[ks][kg 0..3][position 0..Qpad)[8 bf16]         position 64 w + 32 ct + j holds query 64 w + 2 j + ct
//           (the accumulator column mapping of gemm_filter_kernel, so the shared epilogue applies unchanged); a B
//           fragment is one 16-byte load per lane, straight from L2 into registers NLEAD K-steps ahead.
// Block = 8 waves, tile 128 corpus rows x 512 queries; LDS ring of kBfStages stages, DMA kBfStages-2 steps ahead;
// every step issues the same VMEM sequence (1 DMA, then 2 + 2 query loads), so all vmcnt waits are constants.
// tools/bf16_filter_probe.hip is this K-loop without the epilogue: 8.9 ms for the C2 GEMM (1.77 PFLOP/s).
//
// LIMBS = 3: the f32 GEMM engine's TIGHT filter as a split-bf16 GEMM. Every value is written x = h + l + r with
// h = rne_bf16(x), l = rne_bf16(x - h) (x - h is exact in f32, |r| <= 2^-16 |x|); the kernel accumulates qh.vh + qh.vl + ql.vh,
// three bf16 products per dimension, each exact in f32. The corpus lo limbs live in a second copy (kCopyBfDotLo / kCopyBfCosLo) of the hi copy's exact layout, the
// query lo limbs in a second Bb block right behind the first. A stage carries both 8-KiB corpus pieces (16 KiB, 8 stages =
// 128 KiB of LDS); a step issues 2 DMA + 2 x 4 query loads (hi, hi, lo, lo per depth) -- still the same sequence every step.
#pragma once

#include "kernels_gemm.h"

namespace innr {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x4s __attribute__((ext_vector_type(4)));

constexpr int kBfStages = 8, kBfLead = 2, kBfStageBytes = 8192, kBfWaves = 8, kBfK = 32;
static_assert(kBfStages == 8 && kBfLead == 2, "the one-barrier-per-two-steps schedule is derived for an 8-stage ring and a 2-step register ring");

// round-to-nearest-even f32 -> bf16 (NaN stays NaN, quieted)
__device__ __forceinline__ uint16_t f32_to_bf16_rne(float x) {
    uint32_t b = __float_as_uint(x);
    if ((b & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((b >> 16) | 0x40u);
    b += 0x7fffu + ((b >> 16) & 1u);
    return (uint16_t)(b >> 16);
}

// limb l of x as a sum of bf16 values: x = limb0 + limb1 + limb2 up to 2^-24 |x| (each difference below is exact in f32)
__device__ __forceinline__ uint16_t bf16_limb(float x, int l) {
    uint16_t h = f32_to_bf16_rne(x);
    for (int t = 0; t < l; ++t) {
        x -= __uint_as_float((uint32_t)h << 16);
        h = f32_to_bf16_rne(x);
    }
    return h;
}
constexpr uint32_t kBfL2Extra = 6;  // the squared-L2 copy's additional K columns
// errflag words [32, 36) of the screened split filter: wave tiles that flagged something, their flagged sub-tiles, the (row, query)
// pairs corrected one by one (the pair path), and the wave tiles that flagged more than kPairCap pairs (the MFMA fallback)
constexpr uint32_t kScreenCountWord = 32;
// P: the most flagged pairs of one wave tile that the pair path corrects (DESIGN.md 4.4e has the sweep over 8 / 16 / 32)
#ifndef INNR_PAIR_CAP
#define INNR_PAIR_CAP 16
#endif
constexpr int kPairCap = INNR_PAIR_CAP;
static_assert(kPairCap >= 2 && kPairCap <= 64, "a queue entry's slot is a count of flagged lanes; the queue is a few LDS words per wave");
// pairs whose loads are in flight behind one wait. ONE: with two (64 registers beside the 128 accumulators and the K-loop's operand
// ring) the allocator spills 65 registers, the in-flight ring among them (tools/check_gemm_asm.py fails)
constexpr int kPairNP = 1;
static_assert(kPairCap % kPairNP == 0, "the finish loop takes the queue kPairNP entries at a time");
constexpr size_t kPairMaxQpad = (size_t)1 << 20;  // split_pair_delta: 128 query units of Qpad x 16 bytes are a 32-bit lane offset

// one thread per 16-byte output unit (8 dimensions of one corpus row)
// limb: 0 = the rounded values (the hi limb: kCopyBfDot / -Cos / -L2), 1 = their lo limbs (kCopyBfDotLo / -CosLo, the split filter; not with sqn)
// rowscale (nullable): 1/||v|| per row (0 for zero-norm rows) -- the COSINE copy holds the normalised rows, so that the plain
// dot of the filter kernel IS the approximate cosine (with the queries normalised the same way) and no norm is loaded per tile
// sqn (nullable): |v|^2 per row -- the SQUARED-L2 copy carries six more K columns per row, [three bf16 limbs of |v|^2, 1, 1, 1],
// against [-1, -1, -1, three limbs of c_j] and DOUBLED queries on the other side: the plain dot of the filter kernel is then
// 2 q.v - |v|^2 + c_j = C_j - |q - v|^2 up to rounding (c_j = C_j - |q_j|^2 >= 0 as for kGemmL2, kernels_gemm.h), no norm is
// loaded per tile and the score is non-negative where it matters (the raw-bit fast reject of the epilogue)
__global__ __launch_bounds__(256) void pack_corpus_bf16_kernel(const float* __restrict__ V, size_t ldN, uint32_t N, uint32_t D,
                                                                uint32_t nk, size_t units, uint4* __restrict__ Ab,
                                                                const float* __restrict__ rowscale = nullptr,
                                                                const float* __restrict__ sqn = nullptr, int limb = 0) {
    const size_t u = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= units) return;
    const uint32_t i = (uint32_t)(u & 31), rt = (uint32_t)((u >> 5) & 3), kg = (uint32_t)((u >> 7) & 3);
    const size_t tk = u >> 9;  // tile * nk + ks
    const uint32_t ks = (uint32_t)(tk % nk);
    const size_t row = (tk / nk) * 128 + 4 * i + rt;
    const float rs = (rowscale && row < N) ? rowscale[row] : 1.0f;
    uint16_t h[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint32_t d = ks * 32 + kg * 8 + e;
        h[e] = (row < N && d < D) ? bf16_limb(V[(size_t)d * ldN + row] * rs, limb) : (uint16_t)0;
        if (sqn && row < N && d >= D && d < D + kBfL2Extra)
            h[e] = (d - D < 3) ? bf16_limb(sqn[row], (int)(d - D)) : (uint16_t)0x3F80u;  // limbs of |v|^2, then 1.0 three times
    }
    uint4 o;
    o.x = h[0] | ((uint32_t)h[1] << 16); o.y = h[2] | ((uint32_t)h[3] << 16);
    o.z = h[4] | ((uint32_t)h[5] << 16); o.w = h[6] | ((uint32_t)h[7] << 16);
    Ab[u] = o;
}

// a non-negative double rounded UP to float (NaN stays NaN, +inf stays +inf)
__device__ __forceinline__ float f32_round_up(double x) {
    float f = (float)x;
    if ((double)f < x) f = __uint_as_float(__float_as_uint(f) + 1u);
    return f;
}

// The largest limb norms of the split filter's corpus copies (the screen margin, api.hip split_screen_scale): out[0] = bits of
// max_i |vh_i|, out[1] = bits of max_i |vl_i| over the rows i < N, with vh / vl exactly the limbs pack_corpus_bf16_kernel writes
// (bf16_limb(V[d ldN + row] * rs, 0 / 1), d < D; rowscale as there). One pass over the f32 store, one lane = 4 rows (float4 rows,
// coalesced like norms_kernel); a row's sums run in double, the square root is rounded up to float. A block maximum, then
// one atomic max per block and limb on the raw bits (non-negative floats order like their bits; a NaN norm poisons the maximum as in
// norms_kernel, an infinite one stays infinite: the host then keeps the worst-case margin). out is zeroed by the caller.
__global__ __launch_bounds__(256) void limb_maxima_kernel(const float* __restrict__ V, size_t ldN, uint32_t N, uint32_t D,
                                                           const float* __restrict__ rowscale, uint32_t* __restrict__ out) {
    const size_t i4 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    uint32_t hb = 0, lb = 0;
    if (i4 < ldN) {
        float rs[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) rs[c] = (rowscale && i4 + c < N) ? rowscale[i4 + c] : 1.0f;
        const float4* p = reinterpret_cast<const float4*>(V + i4);
        const size_t stride = ldN / 4;
        double sh[4] = {0.0, 0.0, 0.0, 0.0}, sl[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
        for (uint32_t d = 0; d < D; ++d) {
            const float4 v = p[(size_t)d * stride];
            const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float xs = x[c] * rs[c];
                const double h = (double)__uint_as_float((uint32_t)bf16_limb(xs, 0) << 16);
                const double l = (double)__uint_as_float((uint32_t)bf16_limb(xs, 1) << 16);
                sh[c] += h * h;
                sl[c] += l * l;
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (i4 + c >= N) continue;
            const float nh = f32_round_up(sqrt(sh[c])), nl = f32_round_up(sqrt(sl[c]));
            const uint32_t bh = nh != nh ? 0x7fc00000u : __float_as_uint(nh), bl = nl != nl ? 0x7fc00000u : __float_as_uint(nl);
            hb = hb > bh ? hb : bh;
            lb = lb > bl ? lb : bl;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t oh = (uint32_t)__shfl_xor((int)hb, off, 64), ol = (uint32_t)__shfl_xor((int)lb, off, 64);
        hb = hb > oh ? hb : oh;
        lb = lb > ol ? lb : ol;
    }
    __shared__ uint32_t wmax[2][4];
    if ((threadIdx.x & 63) == 0) {
        wmax[0][threadIdx.x >> 6] = hb;
        wmax[1][threadIdx.x >> 6] = lb;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const uint32_t* w = wmax[threadIdx.x];
        const uint32_t a = w[0] > w[1] ? w[0] : w[1], b = w[2] > w[3] ? w[2] : w[3];
        atomicMax(out + threadIdx.x, a > b ? a : b);
    }
}

// queries row-major [Q][D] -> Bb; one thread per 16-byte unit
// l2c (nullable; [Qpad] c_j = C_j - |q_j|^2): the squared-L2 packing, see pack_corpus_bf16_kernel
// limb: 0 = the rounded values (hi limb), 1 = their lo limbs (the split filter; not with l2c)
__global__ __launch_bounds__(256) void pack_queries_bf16_kernel(const float* __restrict__ Qm, uint32_t Q, uint32_t D, uint32_t nk,
                                                                 uint32_t Qpad, uint4* __restrict__ Bb,
                                                                 const float* __restrict__ qscale = nullptr,
                                                                 const float* __restrict__ l2c = nullptr, int limb = 0) {
    const size_t u = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= (size_t)nk * 4 * Qpad) return;
    const uint32_t pos = (uint32_t)(u % Qpad);
    const uint32_t kk = (uint32_t)(u / Qpad);  // ks * 4 + kg
    const uint32_t q = (pos & ~63u) + 2 * (pos & 31) + ((pos >> 5) & 1);
    const float qs = l2c ? 2.0f : ((qscale && q < Q) ? qscale[q] : 1.0f);  // cosine: 1/||q|| (0 below the reference's epsilon)
    uint16_t h[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint32_t d = kk * 8 + e;
        h[e] = (q < Q && d < D) ? bf16_limb(Qm[(size_t)q * D + d] * qs, limb) : (uint16_t)0;
        if (l2c && q < Q && d >= D && d < D + kBfL2Extra)
            h[e] = (d - D < 3) ? (uint16_t)0xBF80u : bf16_limb(l2c[q], (int)(d - D - 3));  // -1.0 three times, then limbs of c_j
    }
    uint4 o;
    o.x = h[0] | ((uint32_t)h[1] << 16); o.y = h[2] | ((uint32_t)h[3] << 16);
    o.z = h[4] | ((uint32_t)h[5] << 16); o.w = h[6] | ((uint32_t)h[7] << 16);
    Bb[u] = o;
}

__device__ __forceinline__ const char* uniform_ptr(const char* p) {  // pin a wave-uniform pointer into SGPRs
    const uint64_t v = (uint64_t)p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return (const char*)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ void gload4(u32x4_t& dst, const char* base_uniform, uint32_t lane_off) {
    uint64_t base;  // s_mov_b64 first: see gload2 (kernels_gemm.h)
    asm volatile("s_mov_b64 %1, %3\n\tglobal_load_dwordx4 %0, %2, %1" : "=v"(dst), "=&s"(base) : "v"(lane_off), "s"(base_uniform) : "memory");
}
template <int N> __device__ __forceinline__ void use_after(u32x4_t& a, u32x4_t& b) {
    asm volatile("s_waitcnt vmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N));
}

// per-step geometry of the K-loop: corpus pieces per stage (hi, + lo for the split filter), and the VMEM ops a wave issues per
// step in their fixed order -- kDma LDS-DMA pieces, then kLoads query loads after each of the two depths' MFMAs
template <int LIMBS> struct BfGeom {
    static_assert(LIMBS == 1 || LIMBS == 3, "one bf16 limb (the bf16 filter) or the split hi.hi + hi.lo + lo.hi (the f32 engine's filter)");
    static constexpr int kParts = LIMBS == 3 ? 2 : 1;
    static constexpr int kStage = kParts * kBfStageBytes;
    static constexpr int kDma = kParts, kLoads = 2 * kParts, kPerStep = kDma + 2 * kLoads;
};

template <int LIMBS>
struct alignas(16) GemmBf16Lds {
    alignas(16) char A[kBfStages * BfGeom<LIMBS>::kStage];
    uint32_t cnt[64 * kBfWaves];
    uint32_t thr[64 * kBfWaves];
};

// The screen's threshold of one query as raw float bits: the sub-tile's best hi.hi score, compared as a signed int, must reach it
// for the sub-tile to be corrected. key: the query's threshold as an order key, m: its screen margin (>= 0, +inf: no screening).
// thr - m is rounded to nearest and then taken one place down, so the result is never above the real difference.
__device__ __forceinline__ int32_t screen_raw(uint32_t key, float m) {
    if (!(key & 0x80000000u)) return INT32_MIN;  // no usable non-negative bound: everything is corrected
    const uint32_t bits = key & 0x7fffffffu;
    if (bits > 0x7f800000u) return INT32_MAX;    // a closed query (padding: the largest key): nothing reaches it
    const float t = __uint_as_float(bits) - m;
    if (!(t > 0.0f)) return INT32_MIN;           // (also inf - inf)
    return (int32_t)__float_as_uint(t) - 1;
}

// The split filter's two small products of single (corpus row, query) pairs, qh.vl + ql.vh, by the whole wave from global memory:
// out[p] for NP pairs at once (NP x 2 units x 4 loads in flight behind one wait, 32 NP registers; the screened kernel takes its
// queue kPairNP pairs at a time). tile / row: the corpus row 128 tile + row (row 0..127), pos: the query's position within Qpad (position
// 64 w + 32 ct + j holds query 64 w + 2 j + ct). A pair is 4 nk 16-byte units (K-step ks, group kg: u = 4 ks + kg) of each of the
// four limb vectors, addressed as the pack kernels above write them: corpus ((tile nk + ks) 8192 + kg 2048 + (row % 4) 512 +
// (row / 4) 16, the same in Ab and Abx), queries (u Qpad + pos) 16, the lo limbs nk 4 Qpad 16 bytes behind the hi limbs. Lane l
// takes units l, l + 64 (every row up to D = 1024 in one trip) and so on in trips of 128. bf16 -> f32 is a shift, every product
// is exact, the 2D of them are summed in f32: another order of the sum the MFMA correction forms, within the same bound (4.4e).
// Plain loads: the compiler waits for them. The result is the same in every lane.
template <int NP>
__device__ __forceinline__ void split_pair_delta(const char* __restrict__ Ab, const char* __restrict__ Abx, const char* __restrict__ Bb,
                                                 const uint32_t (&tile)[NP], const uint32_t (&row)[NP], const size_t (&pos)[NP], uint32_t nk,
                                                 size_t Qpad, int lane, float (&out)[NP]) {
    const uint32_t nu = 4 * nk;
    const size_t b_lo = (size_t)nu * Qpad * 16;
    const uint32_t q_unit = (uint32_t)Qpad * 16u;  // (128 of them fit 32 bits: kPairMaxQpad)
    float sum[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) sum[p] = 0.0f;
    for (uint32_t u0 = 0; u0 < nu; u0 += 128) {
        // every address is a wave-uniform base (the pair, the trip) plus a 32-bit lane offset (the unit): no address registers
        const char *pv[NP], *pl[NP], *pq[NP], *pql[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const size_t ao = (size_t)tile[p] * nk * kBfStageBytes + (size_t)((row[p] & 3) * 512 + (row[p] >> 2) * 16);
            pv[p] = uniform_ptr(Ab + ao);
            pl[p] = uniform_ptr(Abx + ao);
            pq[p] = uniform_ptr(Bb + ((size_t)u0 * Qpad + pos[p]) * 16);
            pql[p] = uniform_ptr(Bb + b_lo + ((size_t)u0 * Qpad + pos[p]) * 16);
        }
        u32x4_t vh[NP][2], vl[NP][2], qh[NP][2], ql[NP][2];
        bool live[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint32_t u = u0 + 64 * j + (uint32_t)lane;
            live[j] = u < nu;
            const uint32_t uc = live[j] ? u : nu - 1;  // past the row's end: its last unit again, not summed
            const uint32_t co = (uc >> 2) * (uint32_t)kBfStageBytes + (uc & 3) * 2048u, qo = (uc - u0) * q_unit;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                vh[p][j] = *reinterpret_cast<const u32x4_t*>(pv[p] + co);
                vl[p][j] = *reinterpret_cast<const u32x4_t*>(pl[p] + co);
                qh[p][j] = *reinterpret_cast<const u32x4_t*>(pq[p] + qo);
                ql[p][j] = *reinterpret_cast<const u32x4_t*>(pql[p] + qo);
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                float t = 0.0f;
#pragma unroll
                for (int e = 0; e < 4; ++e) {  // two bf16 per word: the low half shifted up, the high half masked
                    t = __builtin_fmaf(__uint_as_float(qh[p][j][e] << 16), __uint_as_float(vl[p][j][e] << 16), t);
                    t = __builtin_fmaf(__uint_as_float(ql[p][j][e] << 16), __uint_as_float(vh[p][j][e] << 16), t);
                    t = __builtin_fmaf(__uint_as_float(qh[p][j][e] & 0xffff0000u), __uint_as_float(vl[p][j][e] & 0xffff0000u), t);
                    t = __builtin_fmaf(__uint_as_float(ql[p][j][e] & 0xffff0000u), __uint_as_float(vh[p][j][e] & 0xffff0000u), t);
                }
                sum[p] += live[j] ? t : 0.0f;
            }
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) sum[p] += __shfl_xor(sum[p], off, 64);
        out[p] = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(sum[p])));
    }
}

// row within its 32 x 32 sub-tile of a queue entry (lane | g << 6 | ct << 10 | rt << 11) of the screened kernel: the MFMA's output layout
__device__ __forceinline__ uint32_t prow_in_subtile(uint32_t en) {
    const uint32_t g = (en >> 6) & 15;
    return (g & 3) + 8 * (g >> 2) + 4 * ((en >> 5) & 1);
}

#ifdef INNR_TEST_HOOKS
// innrdbg_split_pair_scores: split_pair_delta as the screened kernel calls it (kPairNP pairs per call), one wave per kPairNP
// caller-given pairs; pairs[2 i] = corpus row, pairs[2 i + 1] = query (both checked by the host), out[i] = qh.vl + ql.vh of pair i
__global__ __launch_bounds__(64) void split_pair_scores_kernel(const char* __restrict__ Ab, const char* __restrict__ Abx, const char* __restrict__ Bb,
                                                               uint32_t nk, size_t Qpad, const uint32_t* __restrict__ pairs, uint32_t n,
                                                               float* __restrict__ out) {
    const uint32_t i0 = kPairNP * blockIdx.x;
    uint32_t tile[kPairNP], row[kPairNP];
    size_t pos[kPairNP];
#pragma unroll
    for (int p = 0; p < kPairNP; ++p) {
        const uint32_t i = i0 + p < n ? i0 + p : n - 1;
        const uint32_t r = pairs[2 * i], q = pairs[2 * i + 1];
        tile[p] = r / 128;
        row[p] = r % 128;
        pos[p] = (q & ~63u) + 32 * (q & 1) + ((q & 63) >> 1);
    }
    float d[kPairNP];
    split_pair_delta<kPairNP>(Ab, Abx, Bb, tile, row, pos, nk, Qpad, (int)threadIdx.x, d);
#pragma unroll
    for (int p = 0; p < kPairNP; ++p)
        if (threadIdx.x == (uint32_t)p && i0 + p < n) out[i0 + p] = d[p];
}
#endif

// MODE 0: fused top-k filter. MODE 1: dump the dense score matrix (layout test).
// LIMBS 1: the bf16 filter (Abx unused). LIMBS 3: the split filter -- Abx the corpus' lo-limb copy, Bb holds nk K-steps of query hi
// limbs followed by nk K-steps of lo limbs.
// SCREEN (LIMBS 3, MODE 0 only): the K-loop is the LIMBS = 1 loop -- hi.hi alone, the lo copies untouched. At the
// end of a tile every 32 x 32 sub-tile whose best hi.hi score stays more than the queries' screen margin (gthr + 2 Qpad: a bound of
// |qh.vl + ql.vh| and of their accumulation) below the threshold is rejected as its full score would have been; to the others the
// wave alone adds the two small products from global memory, and the shared epilogue runs on the full split scores. Lists up to 64
// (R <= 8): a wave tile with at most kPairCap (row, query) pairs at thr - m corrects exactly those pairs, each by the whole wave in
// one memory round trip (split_pair_delta); a wave tile with more keeps the MFMA correction of its flagged sub-tiles.
// MODE 3 (LIMBS 3, SCREEN 0, R 6 only): the split filter's SEEDER over a corpus prefix of whole tiles, one tile per block
// (tiles_per_slice = 1). The full three-product K-loop, no thresholds, no lists: the epilogue writes, per query column and row
// tile rt, the best split score of the 32 rows 128 tile + 4 i + rt as an order key to dump[(4 tile + rt) ld_dump + query]
// (uint32_t words); split_seed_kernel below turns a query's column of them into its first chip-wide bound.
template <int R, int MODE, int LIMBS, int SCREEN = 0>
__global__ __launch_bounds__(64 * kBfWaves, 1) void gemm_bf16_filter_kernel(
    const char* __restrict__ Ab, const char* __restrict__ Abx, const char* __restrict__ Bb, uint32_t ntiles, uint32_t N, uint32_t nk, size_t Qpad, uint32_t nqt,
    uint32_t qtg, uint32_t tiles_per_slice, uint64_t* __restrict__ lists, uint32_t* __restrict__ counts, uint32_t KP, uint32_t kk,
    uint32_t* __restrict__ errflag, uint32_t* gslots, uint32_t* gthr, float* __restrict__ dump, size_t ld_dump) {
    const float* const kmargin = reinterpret_cast<const float*>(gthr + Qpad);  // 2E per query: the k rule of topk_dev.h
    constexpr bool COS = false, U8 = false, L2K = false;  // kind flags of the shared epilogue: plain dot scores
    const float* const invn = nullptr;
    const float* const invq = nullptr;
    const float scale = 1.0f;
    const float iq_lane[2] = {1.0f, 1.0f};
    constexpr int kBQ = 64 * kBfWaves;
    constexpr bool kScreen = SCREEN != 0;
    constexpr bool kPairPath = kScreen && R <= 8;  // lists up to 64: the longer lists' kernels have no room for it
    static_assert(!kScreen || (LIMBS == 3 && MODE == 0), "the screen belongs to the split filter's top-k mode");
    static_assert(MODE != 3 || (LIMBS == 3 && !kScreen && R == 6), "the seeder is the split filter's full loop; its list geometry plays no part");
    constexpr int kLoop = kScreen ? 1 : LIMBS;  // limbs the K-loop multiplies
    using G = BfGeom<kLoop>;
    constexpr bool kSplit = kLoop == 3;
    // gemm_epilogue.inc: nothing this wave still prefetches is waited for. Split filter: the oldest op still needed at the epilogue
    // (end of step s+1) is the DMA of step s+2, issued at the top of step s-4: six whole steps of ops from it on.
    constexpr int kEpiTgWait = kSplit ? G::kPerStep * (kBfStages - 2) : 5 * (kBfStages - 3) + 4 + 5;
    static_assert(kEpiTgWait <= 63 && G::kPerStep * (kBfStages - 4) + G::kPerStep - G::kDma <= 63, "vmcnt is 6 bits");
    constexpr uint32_t kEpiPubEvery = kScreen ? kScreenPubEvery : kPubEvery;  // gemm_epilogue.inc: the publish cadence
    __shared__ GemmBf16Lds<kLoop> s;
    constexpr uint32_t cap = 64 * R;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wu = __builtin_amdgcn_readfirstlane(w);
    // block -> (slice, query tile): as in gemm_filter_kernel
    const uint32_t b = blockIdx.x;
    const uint32_t xcd = b & 7, lb = b >> 3, groups = nqt / qtg;
    const uint32_t qt = (xcd % groups) * qtg + lb % qtg;
    const uint32_t slice = (lb / qtg) * (8 / groups) + xcd / groups;
    const size_t q0 = (size_t)qt * kBQ;
    uint32_t t0 = slice * tiles_per_slice, t1 = t0 + tiles_per_slice;
    if (t1 > ntiles) t1 = ntiles;
    if (t0 > t1) t0 = t1;
    const uint32_t total = (t1 - t0) * nk;

    s.cnt[threadIdx.x] = 0;
    s.thr[threadIdx.x] = 0;
    uint64_t* my_lists = lists + ((size_t)slice * Qpad + q0) * cap;
    float smarg[2] = {0.0f, 0.0f};  // screen margin of this lane's two queries: they never change
    if (kScreen) {
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) smarg[ct] = reinterpret_cast<const float*>(gthr + 2 * Qpad)[q0 + 64 * w + 2 * (lane & 31) + ct];
    }

    f32x16 acc[4][2];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[rt][ct][g] = 0.0f;

    // operand addresses: wave-uniform base + constant lane offset
    const char* sa = Ab + (size_t)t0 * nk * kBfStageBytes + (size_t)wu * 1024;  // this wave's 1-KiB piece of step 0
    const char* sx = kSplit ? Abx + (size_t)t0 * nk * kBfStageBytes + (size_t)wu * 1024 : nullptr;  // ... of the lo limbs
    const uint32_t va = (uint32_t)lane * 16u;
    const uint32_t lds0 = lds_addr_uniform(&s.A[0]) + (uint32_t)wu * 1024u;
    const size_t b_step = (size_t)4 * Qpad * 16, b_depth = (size_t)2 * Qpad * 16, b_ct = 32 * 16, b_lo = (size_t)nk * b_step;
    const char* sb = Bb + (q0 + (size_t)wu * 64) * 16;
    const uint32_t vb = ((uint32_t)(lane >> 5) * (uint32_t)Qpad + (uint32_t)(lane & 31)) * 16u;
    uint32_t a_issued = 0, b_ks = 0;
    const uint32_t last = total ? total - 1 : 0;
    auto issue_a = [&]() {  // DMA of step a_issued; past the end of the slice: the last step again, into a stage nobody reads
        const uint32_t st = a_issued < total ? a_issued : last;
        const uint32_t slot = lds0 + (a_issued % kBfStages) * G::kStage;
        glds16(uniform_ptr(sa + (size_t)st * kBfStageBytes), va, slot);
        if (kSplit) glds16(uniform_ptr(sx + (size_t)st * kBfStageBytes), va, slot + kBfStageBytes);
        ++a_issued;
    };
    constexpr int kB = 2 * G::kParts;  // B fragment registers per depth: [hi ct 0, hi ct 1 (, lo ct 0, lo ct 1)]
    auto issue_b = [&](u32x4_t* d, int m) {
        const char* p = uniform_ptr(sb + (size_t)b_ks * b_step + (size_t)m * b_depth);
        gload4(d[0], p, vb);
        gload4(d[1], uniform_ptr(p + b_ct), vb);
        if (kSplit) {
            gload4(d[2], uniform_ptr(p + b_lo), vb);
            gload4(d[3], uniform_ptr(p + b_lo + b_ct), vb);
        }
    };
    u32x4_t breg[kBfLead][2 * kB];  // [step % kBfLead][kB m + (lo ? 2 : 0) + ct]
#pragma unroll
    for (int r = 0; r < kBfLead; ++r)
#pragma unroll
        for (int x = 0; x < 2 * kB; ++x) breg[r][x] = u32x4_t{0u, 0u, 0u, 0u};
    if (total) {
        for (int i = 0; i < kBfStages - 2; ++i) issue_a();
#pragma unroll
        for (int r = 0; r < kBfLead; ++r) {
            issue_b(&breg[r][0], 0);
            issue_b(&breg[r][kB], 1);
            b_ks = (b_ks + 1 == nk) ? 0 : b_ks + 1;
        }
    }
    wait_all();
#pragma unroll
    for (int r = 0; r < kBfLead; ++r)
#pragma unroll
        for (int x = 0; x < 2 * kB; x += 2) use_after<0>(breg[r][x], breg[r][x + 1]);
    if (kScreen) asm volatile("" : "+v"(smarg[0]), "+v"(smarg[1]));  // landed here: no compiler-made wait for them inside the loop
    __syncthreads();

    uint32_t tg_next[2] = {0u, 0u};
    if (MODE == 0) {
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) gload1_agent(tg_next[ct], gthr + q0 + 64 * wu + ct, 8u * (uint32_t)(lane & 31));
    }
    uint32_t tile = t0, ks = 0;
    for (uint32_t step0 = 0; step0 < total; step0 += kBfLead) {
#pragma unroll
        for (int r = 0; r < kBfLead; ++r) {  // register ring position = step % kBfLead: static. nk is even, so total is too.
            const uint32_t step = step0 + r;
            const char* stage = s.A + (step % kBfStages) * G::kStage;
            issue_a();  // step + kBfStages - 2
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                bf16x8_t a[4], al[4];
#pragma unroll
                for (int rt = 0; rt < 4; ++rt) {
                    const int off = ((2 * m + (lane >> 5)) * 128 + rt * 32 + (lane & 31)) * 16;
                    a[rt] = *reinterpret_cast<const bf16x8_t*>(stage + off);
                    if (kSplit) al[rt] = *reinterpret_cast<const bf16x8_t*>(stage + kBfStageBytes + off);
                }
                // ops younger than this depth's operands (loaded kBfLead steps ago, right after the same depth's MFMAs):
                // the rest of that step, kBfLead - 1 whole steps, this step's DMA and (depth 1) depth 0's reload --
                // 8 of the 5 per step (bf16 filter), 16 of the 10 per step (split filter)
                constexpr int kYounger = G::kPerStep * (kBfLead - 1) + G::kDma + G::kLoads;
                u32x4_t* bm = &breg[r][kB * m];
                use_after<kYounger>(bm[0], bm[1]);
                if (kSplit) use_after<kYounger>(bm[2], bm[3]);
                const bf16x8_t b0 = __builtin_bit_cast(bf16x8_t, bm[0]), b1 = __builtin_bit_cast(bf16x8_t, bm[1]);
                if (kSplit) {
                    // the two small products first; eight independent MFMAs between two that feed the same accumulator
                    const bf16x8_t bl0 = __builtin_bit_cast(bf16x8_t, bm[2]), bl1 = __builtin_bit_cast(bf16x8_t, bm[3]);
#pragma unroll
                    for (int rt = 0; rt < 4; ++rt) {
                        acc[rt][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[rt], bl0, acc[rt][0], 0, 0, 0);
                        acc[rt][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[rt], bl1, acc[rt][1], 0, 0, 0);
                    }
#pragma unroll
                    for (int rt = 0; rt < 4; ++rt) {
                        acc[rt][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[rt], b0, acc[rt][0], 0, 0, 0);
                        acc[rt][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[rt], b1, acc[rt][1], 0, 0, 0);
                    }
                }
#pragma unroll
                for (int rt = 0; rt < 4; ++rt) {
                    acc[rt][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[rt], b0, acc[rt][0], 0, 0, 0);
                    acc[rt][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[rt], b1, acc[rt][1], 0, 0, 0);
                }
                issue_b(bm, m);  // the same registers, kBfLead steps ahead
                __builtin_amdgcn_sched_barrier(0);
            }
            b_ks = (b_ks + 1 == nk) ? 0 : b_ks + 1;
            // (a use in the hot loop, no instruction: with the pair path the allocator otherwise spills the margin and reloads it at every
            //  tile's screen behind a full wait, as it does for R = 12 / 20)
            if (kPairPath) asm volatile("" : "+v"(smarg[0]), "+v"(smarg[1]));
            // nk is a multiple of kBfLead, so a tile always ends on the last ring position: ONE copy of the epilogue in
            // the unrolled loop (two copies made the kernel 81 KB, more than the 64 KB instruction cache)
#ifdef INNR_GEMM_PROBE_SKIPEPI  // tools/bf16_epi_probe.hip: the same code, the epilogue never taken (dump == nullptr at run time)
            if (r == kBfLead - 1 && ks + 1 == nk && dump != nullptr) {
#else
            if (r == kBfLead - 1 && ks + 1 == nk) {
#endif
                bool run_epilogue = true;
                if constexpr (kScreen) {
                    // ---- screen: which of the wave's eight 32 x 32 sub-tiles (rt, ct) can still reach their queries' thresholds ----
                    // thr as the epilogue derives it (its own wait, kEpiTgWait of the LIMBS = 1 sequence; a bound read early
                    // is the older, lower one: thresholds only rise, so the epilogue's is never below the screen's)
                    use_after<kEpiTgWait>(tg_next[0], tg_next[1]);
                    int32_t traw[2];
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) {
                        const uint32_t tl = __hip_atomic_load(&s.thr[64 * w + 2 * (lane & 31) + ct], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                        traw[ct] = screen_raw(tl > tg_next[ct] ? tl : tg_next[ct], smarg[ct]);
                    }
                    uint32_t smask = 0;  // bit 2 rt + ct, wave-uniform
#pragma unroll
                    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
                        for (int ct = 0; ct < 2; ++ct) {
                            int32_t best = INT32_MIN;  // raw-bit maximum, as the epilogue's fast reject
#pragma unroll
                            for (int g = 0; g < 16; ++g) {
                                const int32_t raw = (int32_t)__float_as_uint(acc[rt][ct][g]);
                                best = best > raw ? best : raw;
                            }
                            if (__any(best >= traw[ct])) smask |= 1u << (2 * rt + ct);
                        }
                    if (smask == 0) {
                        // nothing of this tile can pass: the epilogue's tail alone. The same two threshold loads as the
                        // epilogue issues, so every tile adds the same VMEM ops behind the K-loop's constant sequence
                        // (more ops behind an awaited one only make a counted wait stricter, fewer never happen).
                        run_epilogue = false;
#pragma unroll
                        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
                            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                                for (int g = 0; g < 16; ++g) acc[rt][ct][g] = 0.0f;
#pragma unroll
                        for (int ct = 0; ct < 2; ++ct) gload1_agent(tg_next[ct], gthr + q0 + 64 * wu + ct, 8u * (uint32_t)(lane & 31));
                    } else {
                        // ---- which PAIRS of the flagged sub-tiles reach thr - m: a per-wave LDS queue of (rt, ct, g, lane) ----
                        // (lists up to 64, kPairPath: the longer lists' kernels have neither the registers nor, at R = 20, the room
                        //  below the 64 KB instruction cache; they correct every flagged wave tile by MFMA as before.)
                        // Wave scope only: the queue and the deltas are this wave's own, LDS operations of a wave complete in
                        // order, no block barrier. One runtime loop over the set bits of smask: the sub-tile's 16 values are
                        // selected into one register tuple (the only code per sub-tile; a static walk over the 128 values,
                        // written out 8 x 16 times, put the kernel past the instruction cache), a lane collects their flags in
                        // a mask, and an inner loop takes every lane's lowest flagged g per trip (one trip unless a lane holds
                        // two flagged values of the sub-tile): a value's slot is the running count plus its lane's rank among
                        // the lanes of the trip. Nothing is written past kPairCap.
                        __shared__ uint32_t pairq[kBfWaves][kPairCap];
                        __shared__ uint2 pairw[kBfWaves][kPairCap];  // a pair's delta as three bf16 limbs
                        // (the lane and wave numbers made opaque here: nothing derived from them for this branch -- LDS addresses,
                        //  lane masks -- is computed ahead of the K-loop and held in registers across it)
                        int ln = lane, wq = wu;
                        asm volatile("" : "+v"(ln), "+s"(wq));
                        uint32_t npair = 0;
#pragma unroll 1
                        for (uint32_t sm = kPairPath ? smask : 0u; sm != 0; sm &= sm - 1) {
                            const uint32_t sidx = (uint32_t)__builtin_ctz(sm);  // 2 rt + ct, wave-uniform
                            f32x16 sv = acc[0][0];  // this sub-tile's 16 values: 16 moves per sub-tile, one code path behind them
#pragma unroll
                            for (int rt = 0; rt < 4; ++rt)
#pragma unroll
                                for (int ct = 0; ct < 2; ++ct)
                                    if (sidx == (uint32_t)(2 * rt + ct)) sv = acc[rt][ct];
                            const int32_t t = (sidx & 1) ? traw[1] : traw[0];
                            uint32_t gm = 0;
#pragma unroll
                            for (int g = 0; g < 16; ++g) gm |= (int32_t)__float_as_uint(sv[g]) >= t ? 1u << g : 0u;
#pragma unroll 1
                            for (unsigned long long fm = __ballot(gm != 0); fm != 0; fm = __ballot(gm != 0)) {
                                const uint32_t slot = npair + __builtin_amdgcn_mbcnt_hi((uint32_t)(fm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)fm, 0u));
                                if (gm != 0 && slot < (uint32_t)kPairCap) pairq[wq][slot] = (uint32_t)ln | (uint32_t)__builtin_ctz(gm) << 6 | sidx << 10;
                                gm &= gm - 1;
                                npair += (uint32_t)__builtin_popcountll(fm);
                            }
                        }
                        const bool by_pairs = kPairPath && npair <= (uint32_t)kPairCap;  // wave-uniform
                        if (ln < 4) {  // words 32 .. 35, one atomic instruction
                            const uint32_t add = ln == 0 ? 1u : ln == 1 ? (uint32_t)__builtin_popcount(smask) : ln == 2 ? (by_pairs ? npair : 0u) : (by_pairs ? 0u : 1u);
                            const uint32_t l4 = 4u * (uint32_t)ln;
                            atomicAdd(reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(errflag + kScreenCountWord) + l4), add);
                        }
                        if (by_pairs) {
                            // ---- pair correction: qh.vl + ql.vh of each queued pair by the whole wave (split_pair_delta), one
                            // memory round trip per kPairNP pairs; the deltas wait in LDS as three bf16 limbs each. They reach
                            // the accumulators in the sub-tile loop below, shared with the MFMA correction: one MFMA per pair on
                            // its sub-tile with A = 1.0 in row i at k = 0, 1, 2 and B = the limbs of d in column j, so exactly
                            // (i, j) receives d1 + d2 + d3 (= d up to 2^-24 |d|, inside the accumulation term of E and of the
                            // margin) and every other value of the sub-tile + 0. (The accumulator tuples change only there, in
                            // place, by MFMA: single elements assigned under a branch, MFMAs under a runtime sub-tile index, or a
                            // second static loop of their own made the register allocator copy and spill the tuples.) An
                            // unflagged value keeps its hi.hi score, below thr - m: rejected as its full score would have been.
                            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                            __builtin_amdgcn_wave_barrier();
                            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll 1
                            for (uint32_t e = 0; e < npair; e += kPairNP) {  // (a ragged end: the last pair again, its delta unused)
                                uint32_t prow[kPairNP], ptile[kPairNP];
                                size_t ppos[kPairNP];
#pragma unroll
                                for (int p = 0; p < kPairNP; ++p) {
                                    const uint32_t en = __builtin_amdgcn_readfirstlane(pairq[wq][e + p < npair ? e + p : npair - 1]);
                                    const uint32_t L = en & 63, g = (en >> 6) & 15;
                                    ptile[p] = tile;
                                    prow[p] = 4 * ((g & 3) + 8 * (g >> 2) + 4 * (L >> 5)) + (en >> 11);  // the epilogue's row of (rt, g, lane)
                                    ppos[p] = q0 + 64 * (size_t)wq + 32 * ((en >> 10) & 1) + (L & 31);
                                }
                                float d[kPairNP];
                                split_pair_delta<kPairNP>(Ab, Abx, Bb, ptile, prow, ppos, nk, Qpad, ln, d);
                                if (ln < kPairNP) {  // (kPairCap is a multiple of kPairNP: e + lane is a slot)
                                    float dl = d[0];
#pragma unroll
                                    for (int p = 1; p < kPairNP; ++p) dl = ln == p ? d[p] : dl;
                                    pairw[wq][e + ln] = uint2{(uint32_t)bf16_limb(dl, 0) | (uint32_t)bf16_limb(dl, 1) << 16, (uint32_t)bf16_limb(dl, 2)};
                                }
                            }
                            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                            __builtin_amdgcn_wave_barrier();
                            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                        }
                        {
                        // ---- per flagged sub-tile: the queued pairs' deltas (by_pairs), or the MFMA correction (more than kPairCap
                        // pairs: near ties, tiles without a bound, long lists): qh.vl + ql.vh of the whole sub-tile, by this wave alone ----
                        // Fragments straight from global memory in the layouts the K-loop reads: A fragment (K-step ks, depth m,
                        // row tile rt) = 64 lanes x 16 B at ((2 m + lane / 32) 128 + 32 rt + lane % 32) 16 of the tile's 8-KiB
                        // piece of step ks (hi: Ab, lo: Abx), B fragment as issue_b addresses it (lo: b_lo behind). Plain loads:
                        // the compiler waits for them itself (no asm load is issued between a load and its use), and these extra
                        // VMEM ops only make the K-loop's counted waits stricter. No barrier.
                        const char* ca = Ab + (size_t)tile * nk * kBfStageBytes;
                        const char* cx = Abx + (size_t)tile * nk * kBfStageBytes;
                        const uint32_t fo = ((uint32_t)(ln >> 5) * 128u + (uint32_t)(ln & 31)) * 16u;
                        const uint32_t vbq = ((uint32_t)(ln >> 5) * (uint32_t)Qpad + (uint32_t)(ln & 31)) * 16u;  // vb, made here
                        constexpr int kCorrSteps = 2;  // K-steps of loads per wait: 16 loads, 64 registers
                        static_assert(kCorrSteps == kBfLead, "nk is a multiple of kBfLead (launch_gemm_split checks it): a batch never leaves the tile");
#pragma unroll
                        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
                            for (int ct = 0; ct < 2; ++ct) {
                                if (!(smask & (1u << (2 * rt + ct)))) continue;  // wave-uniform; the accumulator index is static
                                if (by_pairs) {
#pragma unroll 1
                                    for (uint32_t e = 0; e < npair; ++e) {
                                        const uint32_t en = __builtin_amdgcn_readfirstlane(pairq[wq][e]);
                                        if ((en >> 10) != (uint32_t)(2 * rt + ct)) continue;
                                        const uint2 dw = pairw[wq][e];
                                        const bool ra = (uint32_t)ln == prow_in_subtile(en), cb = (uint32_t)ln == (en & 31);  // lanes 0 .. 31 hold k = 0 .. 7
                                        const u32x4_t fa = {ra ? 0x3F803F80u : 0u, ra ? 0x3F80u : 0u, 0u, 0u};
                                        const u32x4_t fb = {cb ? dw.x : 0u, cb ? dw.y : 0u, 0u, 0u};
                                        acc[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, fa), __builtin_bit_cast(bf16x8_t, fb),
                                                                                              acc[rt][ct], 0, 0, 0);
                                    }
                                    continue;
                                }
                                for (uint32_t k0 = 0; k0 < nk; k0 += kCorrSteps) {
                                    u32x4_t fa[kCorrSteps][2], fl[kCorrSteps][2], fb[kCorrSteps][2], fbl[kCorrSteps][2];
#pragma unroll
                                    for (int j = 0; j < kCorrSteps; ++j)
#pragma unroll
                                        for (int m = 0; m < 2; ++m) {
                                            const size_t ao = (size_t)(k0 + j) * kBfStageBytes + (size_t)((2 * m * 128 + rt * 32) * 16) + fo;
                                            const char* pb = sb + (size_t)(k0 + j) * b_step + (size_t)m * b_depth + (size_t)ct * b_ct + vbq;
                                            fa[j][m] = *reinterpret_cast<const u32x4_t*>(ca + ao);
                                            fl[j][m] = *reinterpret_cast<const u32x4_t*>(cx + ao);
                                            fb[j][m] = *reinterpret_cast<const u32x4_t*>(pb);
                                            fbl[j][m] = *reinterpret_cast<const u32x4_t*>(pb + b_lo);
                                        }
#pragma unroll
                                    for (int j = 0; j < kCorrSteps; ++j)
#pragma unroll
                                        for (int m = 0; m < 2; ++m) {
                                            acc[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                                                __builtin_bit_cast(bf16x8_t, fa[j][m]), __builtin_bit_cast(bf16x8_t, fbl[j][m]), acc[rt][ct], 0, 0, 0);
                                            acc[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                                                __builtin_bit_cast(bf16x8_t, fl[j][m]), __builtin_bit_cast(bf16x8_t, fb[j][m]), acc[rt][ct], 0, 0, 0);
                                        }
                                }
                            }
                        }
                    }
                }
                if (run_epilogue) {
#include "gemm_epilogue.inc"
                }
                ks = 0;
                ++tile;
            } else {
                ++ks;
            }
            // ONE barrier per kLead = 2 K-steps: between two barriers the block reads stages s, s + 1 and its DMAs write the
            // stages of steps s + 6, s + 7 -- last read two steps before the previous barrier, never one of the two in use.
            // At the barrier this wave's pieces of steps s + 2 and s + 3 must have landed: the younger one was issued at the
            // top of step s - 3, with 4 + 5 (STAGES - 4) VMEM ops of this wave behind it (split filter: the lo piece, with
            // 8 + 10 (STAGES - 4); more after an epilogue: the wait is then only stricter). The waves of a SIMD drift apart inside the two-step window instead of meeting at a
            // barrier every 16 MFMAs.
            if (r == kBfLead - 1) {
                wait_but_youngest<G::kPerStep * (kBfStages - 4) + G::kPerStep - G::kDma>();
                __syncthreads();
            }
        }
    }
    wait_all();
    __syncthreads();
    if (MODE == 0) {
        const uint32_t c = __hip_atomic_load(&s.cnt[64 * w + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        unsigned long long need = __ballot(c > KP);
        uint32_t mine = c;
        while (need) {
            const int j = __builtin_ctzll(need);
            need &= need - 1;
            const uint32_t cj = __builtin_amdgcn_readlane(c, j);
            uint32_t t;
            const uint32_t keep = wave_compact<R>(my_lists + (size_t)(64 * w + j) * cap, cj, KP, &t);
            if (lane == j) mine = keep;
        }
        counts[(size_t)slice * Qpad + q0 + 64 * w + lane] = mine;
    }
}

// The split filter's first chip-wide bounds from its seeder's group maxima (MODE 3 above): gmax[ngroups][Qpad] order keys, group g
// of query j = the best split score of 32 prefix rows, the groups disjoint. One wave per query. t = the k-th largest of the
// query's ngroups keys, by bisection on the key bits (as select in gthr_publish_select): the largest t that at least k keys reach.
// At least k DISTINCT rows then have an approximate score >= t -- the certificate of the k rule (topk_dev.h): their exact scores
// are >= t - E, so is the k-th best exact score of the corpus, and a row of the true top k has an approximate score >= t - 2E.
// seed[j] = key(t - 2E) - 1 (one key lower, as seed_thresholds_kernel: the re-score's proof is strict), E = err_scale |q_j| 1.0001
// (cosine: err_scale 1.0001); 0 ("no bound") where that is not finite and for the padding queries j >= Q. The host keeps
// k <= ngroups <= kSeedMaxGroups.
constexpr uint32_t kSeedMaxGroups = 2048;
__global__ __launch_bounds__(64) void split_seed_kernel(const uint32_t* __restrict__ gmax, uint32_t ngroups, uint32_t Qpad, uint32_t Q,
                                                        uint32_t k, int cosine, float err_scale, const float* __restrict__ qnorm,
                                                        uint32_t* __restrict__ seed) {
    __shared__ uint32_t keys[kSeedMaxGroups];
    const uint32_t j = blockIdx.x, lane = threadIdx.x;
    if (j >= Q) {
        if (lane == 0) seed[j] = 0u;
        return;
    }
    for (uint32_t g = lane; g < ngroups; g += 64) keys[g] = gmax[(size_t)g * Qpad + j];
    __syncthreads();
    uint32_t t = 0;
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t cand = t | (1u << bit);
        uint32_t n = 0;  // wave-uniform
        for (uint32_t g0 = 0; g0 < ngroups; g0 += 64) {
            const uint32_t g = g0 + lane;
            n += (uint32_t)__builtin_popcountll(__ballot(g < ngroups && keys[g] >= cand));
        }
#if defined(INNR_MUTATE_SPLIT_SEED) && INNR_MUTATE_SPLIT_SEED == 1  // mutation check, never the product: one rank too high
        if (n + 1 >= k) t = cand;
#else
        if (n >= k) t = cand;
#endif
    }
    if (lane == 0) {
        const float qn = qnorm[j];
#if defined(INNR_MUTATE_SPLIT_SEED) && INNR_MUTATE_SPLIT_SEED == 2  // ... the bound without its 2E
        const float E = 0.0f * err_scale;
#else
        const float E = (cosine ? err_scale : err_scale * qn) * 1.0001f;
#endif
        const float s = ord_f32(t) - 2.0f * E;
        seed[j] = (s - s == 0.0f && qn - qn == 0.0f) ? f32_ord(s) - 1u : 0u;  // (a non-finite query norm: no bound of any kind)
    }
}

}  // namespace innr
