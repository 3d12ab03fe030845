// The loader: one launch turns "batch k0/B of epoch e on rank r" into an int16 (B, n_out) batch, its targets and its clip indices,
// read straight from a device-resident clip bank.  Nothing is read back and no index tensor exists in between.
//   k_loader_indices : the sampling laws alone (DESIGN.md §4 "Loader"), one thread per sample
//   k_loader_batch   : the same draw once per workgroup (thread 0, LDS broadcast), then the copy: 16-byte stores on the aligned
//                      part of the destination row, 16-byte aligned loads + a funnel shift for the source, whose alignment the
//                      crop offset and the row stride decide (any multiple of 2 bytes); head, tail and the chunk that straddles
//                      the end of the clip go element by element
// The laws are integer arithmetic and single IEEE operations: tests/data_pipeline_cases.py restates them bit for bit.
#include "ww_internal.h"

namespace {

constexpr int LD_BLOCK = 256;
constexpr uint32_t TAGW = WW_TAG_DATA << 24;

struct ww_draw {            // by-value description of one rank's sample stream
    const double *cdf;      // WW_SAMPLER_TABLE: inclusive cumulative weights, n_cdf entries, cdf[n_cdf-1] = total > 0
    int32_t n_cdf;
    int32_t n;              // clips
    int32_t strategy, shuffle;
    int32_t half;           // WW_SAMPLER_PERM: half the Feistel width, 2^(2 half) >= max(n, 4)
    uint32_t rank, world;
    uint32_t epoch_lo, seed_lo, seed_hi;
    uint64_t k0;            // first sample of the launch, counted per rank within the epoch
};

// perm_epoch(g): 4-round balanced Feistel over 2*half bits, cycle-walked into [0, n).  g < n, so the walk returns
__device__ inline uint32_t perm_index(const ww_draw &d, uint32_t g) {
    const uint32_t mask = (1u << d.half) - 1u;
    uint32_t x = g;
    do {
        uint32_t l = x >> d.half, r = x & mask;
#pragma unroll 1
        for (uint32_t j = 0; j < 4; ++j) {
            uint32_t o[4];
            ww_philox(r, j, d.epoch_lo, TAGW, d.seed_lo, d.seed_hi, o);
            const uint32_t t = l ^ (o[0] & mask);
            l = r;
            r = t;
        }
        x = (l << d.half) | r;
    } while (x >= (uint32_t)d.n);
    return x;
}

// first i with cdf[i] > u * total, u a 53-bit uniform in [0, 1); a flat stretch of the table (zero weight) is never the first
__device__ inline uint32_t table_index(const ww_draw &d, uint64_t g) {
    uint32_t o[4];
    ww_philox((uint32_t)g, (uint32_t)(g >> 32), d.epoch_lo, TAGW | 1u, d.seed_lo, d.seed_hi, o);
    const uint64_t u53 = (((uint64_t)o[0] << 32) | o[1]) >> 11;
    const double target = __dmul_rn(__dmul_rn((double)u53, 0x1p-53), d.cdf[d.n_cdf - 1]);
    int lo = 0, hi = d.n_cdf;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (d.cdf[mid] > target) hi = mid; else lo = mid + 1;
    }
    return (uint32_t)(lo < d.n_cdf ? lo : d.n_cdf - 1);
}

__device__ inline uint32_t draw_index(const ww_draw &d, uint64_t g) {
    if (d.strategy == WW_SAMPLER_TABLE) return table_index(d, g);
    return d.shuffle ? perm_index(d, (uint32_t)g) : (uint32_t)g;
}

__global__ __launch_bounds__(LD_BLOCK) void k_loader_indices(ww_draw d, int count, int32_t *__restrict__ out) {
    const int i = blockIdx.x * LD_BLOCK + threadIdx.x;
    if (i >= count) return;
    const uint64_t g = (uint64_t)d.rank + (uint64_t)d.world * (d.k0 + (uint64_t)i);
    out[i] = (int32_t)draw_index(d, g);
}

// S workgroups per sample; workgroup s of a sample takes the 16-byte chunks s*256 + tid, + S*256, ...
__global__ __launch_bounds__(LD_BLOCK) void k_loader_batch(const int16_t *__restrict__ bank, const int32_t *__restrict__ length,
                                                           const uint8_t *__restrict__ label, long long L, long long bank_elems,
                                                           ww_draw d, int training, int n_out, int S, int16_t *__restrict__ out,
                                                           int64_t *__restrict__ targets, int32_t *__restrict__ clip_index) {
    __shared__ uint32_t s_idx, s_off, s_ncopy;
    const int tid = threadIdx.x;
    const int b = blockIdx.x / S, s = blockIdx.x % S;
    if (tid == 0) {
        const uint64_t g = (uint64_t)d.rank + (uint64_t)d.world * (d.k0 + (uint64_t)b);
        const uint32_t idx = draw_index(d, g);
        long long len = length[idx];
        len = len < 0 ? 0 : (len > L ? L : len);
        uint32_t off = 0;
        if (len > n_out && training) {
            uint32_t o[4];
            ww_philox((uint32_t)g, (uint32_t)(g >> 32), d.epoch_lo, TAGW | 2u, d.seed_lo, d.seed_hi, o);
            off = __umulhi(o[0], (uint32_t)(len - n_out + 1));
        }
        s_idx = idx;
        s_off = off;
        s_ncopy = (uint32_t)(len < n_out ? len : n_out);
        if (s == 0) {
            targets[b] = (int64_t)label[idx];
            clip_index[b] = (int32_t)idx;
        }
    }
    __syncthreads();
    const int ncopy = (int)s_ncopy;
    const int16_t *src = bank + ((long long)s_idx * L + (long long)s_off);     // 64-bit: n_clips * L passes 2^31
    int16_t *dst = out + (long long)b * n_out;
    // dst[0, head) up to the first 16-byte boundary, nch whole chunks, then the tail
    const int to_align = (int)(((16u - (unsigned)((uintptr_t)dst & 15u)) & 15u) >> 1);
    const int head = to_align < n_out ? to_align : n_out;
    const int nch = (n_out - head) >> 3;
    const int tail0 = head + nch * 8;
    if (s == 0) {
        if (tid < head) {
            dst[tid] = tid < ncopy ? src[tid] : (int16_t)0;
        } else if (tid >= 8 && tid < 8 + (n_out - tail0)) {
            const int e = tail0 + tid - 8;
            dst[e] = e < ncopy ? src[e] : (int16_t)0;
        }
    }
    const uintptr_t sa0 = (uintptr_t)(src + head);             // source address of chunk 0; + 16 per chunk: one shift for all
    const unsigned sh = (unsigned)(sa0 & 15u);                 // bytes, even
    const unsigned ws = sh >> 2, bs = (sh & 3u) * 8u;          // whole words, then 0 or 16 bits
    const uintptr_t bank_lo = (uintptr_t)bank, bank_hi = (uintptr_t)(bank + bank_elems);
    for (int c = s * LD_BLOCK + tid; c < nch; c += S * LD_BLOCK) {
        const int e = head + c * 8;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (e < ncopy) {
            const uintptr_t a0 = (sa0 + (uintptr_t)c * 16u) & ~(uintptr_t)15u;
            // the aligned window [a0, a0 + 16 or 32) holds the 8 samples; it may reach into the neighbouring clips, never
            // outside the bank
            if (e + 8 <= ncopy && a0 >= bank_lo && a0 + (sh ? 32u : 16u) <= bank_hi) {
                const uint4 p = *reinterpret_cast<const uint4 *>(a0);
                if (sh == 0) {
                    v = p;
                } else {
                    const uint4 q = *reinterpret_cast<const uint4 *>(a0 + 16u);
                    const uint32_t x0 = ws == 0 ? p.x : ws == 1 ? p.y : ws == 2 ? p.z : p.w;
                    const uint32_t x1 = ws == 0 ? p.y : ws == 1 ? p.z : ws == 2 ? p.w : q.x;
                    const uint32_t x2 = ws == 0 ? p.z : ws == 1 ? p.w : ws == 2 ? q.x : q.y;
                    const uint32_t x3 = ws == 0 ? p.w : ws == 1 ? q.x : ws == 2 ? q.y : q.z;
                    const uint32_t x4 = ws == 0 ? q.x : ws == 1 ? q.y : ws == 2 ? q.z : q.w;
                    v.x = __funnelshift_r(x0, x1, bs);         // (x1:x0) >> bs, low word
                    v.y = __funnelshift_r(x1, x2, bs);
                    v.z = __funnelshift_r(x2, x3, bs);
                    v.w = __funnelshift_r(x3, x4, bs);
                }
            } else {
                uint32_t h[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) h[j] = e + j < ncopy ? (uint32_t)(uint16_t)src[e + j] : 0u;
                v = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
            }
        }
        *reinterpret_cast<uint4 *>(dst + e) = v;
    }
}

int fill_draw(const char *who, ww_draw &d, int n_clips, int strategy, int shuffle, const double *cdf, int n_cdf, uint64_t seed,
              uint64_t epoch, int rank, int world, int64_t k0, int count) {
    WW_REQUIRE(n_clips >= 1, WW_E_INVALID, "%s: n_clips=%d", who, n_clips);
    WW_REQUIRE(world >= 1 && rank >= 0 && rank < world, WW_E_INVALID, "%s: rank %d of world %d", who, rank, world);
    WW_REQUIRE(k0 >= 0 && count >= 1, WW_E_INVALID, "%s: k0=%lld count=%d", who, (long long)k0, count);
    WW_REQUIRE(strategy == WW_SAMPLER_PERM || strategy == WW_SAMPLER_TABLE, WW_E_INVALID, "%s: unknown strategy %d", who, strategy);
    if (strategy == WW_SAMPLER_TABLE) {
        WW_REQUIRE(cdf && n_cdf >= 1 && n_cdf <= n_clips, WW_E_INVALID, "%s: the table sampler needs 1 <= n_cdf=%d <= n_clips=%d",
                   who, n_cdf, n_clips);
    } else {
        // a permutation has n entries: the last sample of the launch must be one of them
        const unsigned long long g_last = (unsigned long long)rank + (unsigned long long)world * (unsigned long long)(k0 + count - 1);
        WW_REQUIRE(g_last < (unsigned long long)n_clips, WW_E_INVALID,
                   "%s: sample %lld of rank %d/%d is position %llu of an epoch of %d", who, (long long)(k0 + count - 1), rank, world,
                   g_last, n_clips);
    }
    int half = 1;
    while ((1ull << (2 * half)) < (unsigned long long)n_clips) ++half;
    d.cdf = cdf;
    d.n_cdf = n_cdf;
    d.n = n_clips;
    d.strategy = strategy;
    d.shuffle = shuffle != 0;
    d.half = half;
    d.rank = (uint32_t)rank;
    d.world = (uint32_t)world;
    d.epoch_lo = (uint32_t)epoch;
    d.seed_lo = (uint32_t)seed;
    d.seed_hi = (uint32_t)(seed >> 32);
    d.k0 = (uint64_t)k0;
    return WW_OK;
}

}  // namespace

extern "C" int ww_loader_indices(ww_ctx *ctx, int n_clips, int strategy, int shuffle, const double *cdf, int n_cdf, uint64_t seed,
                                 uint64_t epoch, int rank, int world, int64_t k0, int count, int32_t *index_out,
                                 ww_stream_t stream) {
    WW_REQUIRE(ctx && index_out, WW_E_INVALID, "ww_loader_indices: null argument");
    ww_draw d;
    const int rc = fill_draw("ww_loader_indices", d, n_clips, strategy, shuffle, cdf, n_cdf, seed, epoch, rank, world, k0, count);
    if (rc != WW_OK) return rc;
    hipLaunchKernelGGL(k_loader_indices, dim3((count + LD_BLOCK - 1) / LD_BLOCK), dim3(LD_BLOCK), 0, (hipStream_t)stream, d, count,
                       index_out);
    WW_LAUNCH_CHECK();
    return WW_OK;
}

extern "C" int ww_loader_batch(ww_ctx *ctx, const int16_t *bank, const int32_t *length, const uint8_t *label, int n_clips, int L,
                               int strategy, int shuffle, int training, const double *cdf, int n_cdf, uint64_t seed,
                               uint64_t epoch, int rank, int world, int64_t k0, int B, int n_out, int16_t *out, int64_t *targets,
                               int32_t *clip_index, ww_stream_t stream) {
    WW_REQUIRE(ctx && bank && length && label && out && targets && clip_index, WW_E_INVALID, "ww_loader_batch: null argument");
    WW_REQUIRE(L >= 1 && n_out >= 1, WW_E_INVALID, "ww_loader_batch: L=%d n_out=%d", L, n_out);
    ww_draw d;
    const int rc = fill_draw("ww_loader_batch", d, n_clips, strategy, shuffle, cdf, n_cdf, seed, epoch, rank, world, k0, B);
    if (rc != WW_OK) return rc;
    static_assert(LD_BLOCK == 256, "ww_loader_plan_rows counts passes of 256 chunks");
    const int S = ww_loader_plan_rows(B, n_out).S;
    WW_REQUIRE((long long)B * S < (1ll << 31), WW_E_INVALID, "ww_loader_batch: B=%d is too large", B);
    hipLaunchKernelGGL(k_loader_batch, dim3((unsigned)(B * S)), dim3(LD_BLOCK), 0, (hipStream_t)stream, bank, length, label,
                       (long long)L, (long long)n_clips * L, d, training != 0, n_out, S, out, targets, clip_index);
    WW_LAUNCH_CHECK();
    return WW_OK;
}
