// bpoly_seg.cuh -- K2's fold over segments: the fold kernel of sponge.cuh with the segment on grid.y and the batch range taken from the segment table
// (segments.cuh), and the conversion to canonical words per segment.
//
// A call may hand its long segments to the matrix cores (bpoly_mfma_seg.cuh), which write those segments' outputs themselves.  Both kernels here then take the same
// length rule the host classified by -- BpolySegSkip: the segments with lo <= length < hi are not theirs -- and neither reads nor writes anything of such a segment
// (with one slice the fold writes into the output and the finish converts it in place: a skipped segment's output stays as the other kernels left it).
#pragma once
#include "sponge.cuh"
#include "segments.cuh"

namespace mb {

struct BpolySegSkip { uint32_t lo, hi; };                         // lo == hi: every segment is folded here
__device__ __forceinline__ bool bpoly_seg_skipped(const BpolySegSkip &sk, uint32_t len) { return len >= sk.lo && len < sk.hi; }

// bpoly_fold_kernel with the segment on grid.y: block (x, s) covers BP_HT `hi` values, 256 `lo` values and slice `slice` of segment s's proofs.
//   partial[s][slice][j] = sum_{b in the slice} H_b[hi] * L_b[lo]      (Montgomery; an empty slice writes zero)
template <int F>
__global__ void __launch_bounds__(256)
bpoly_fold_seg_kernel(BpolyShape sh, uint32_t slices, MsmSegments sg, BpolySegSkip skip, const fe_t *__restrict__ ltab, const fe_t *__restrict__ htab, fe_t *__restrict__ partial) { mb_wave_prio<1>();
    const uint32_t nl = 1u << sh.lb, nh = 1u << sh.hb;
    const uint32_t lo_blocks = (nl + blockDim.x - 1) / blockDim.x;
    const uint32_t hi_tiles = (nh + BP_HT - 1) / BP_HT;
    uint32_t bid = blockIdx.x;
    const uint32_t lo_blk = bid % lo_blocks; bid /= lo_blocks;
    const uint32_t tile = bid % hi_tiles; const uint32_t slice = bid / hi_tiles;
    const uint32_t lo = lo_blk * blockDim.x + threadIdx.x;
    if (lo >= nl) return;
    uint32_t first, len;
    msm_segment_range(sg, blockIdx.y, sh.batch, first, len);
    if (bpoly_seg_skipped(skip, len)) return;
    const uint32_t b0 = first + (uint32_t)((uint64_t)len * slice / slices);
    const uint32_t b1 = first + (uint32_t)((uint64_t)len * (slice + 1) / slices);
    fe_t acc[BP_HT];
#pragma unroll
    for (int t = 0; t < BP_HT; ++t) acc[t] = fe_zero();
    uint32_t b = b0;
    for (; b + 3 <= b1; b += 3) {                          // three proofs per step: one reduction per dot product
        const fe_t l0 = ltab[(size_t)b * nl + lo], l1 = ltab[(size_t)(b + 1) * nl + lo], l2 = ltab[(size_t)(b + 2) * nl + lo];
#pragma unroll
        for (int t = 0; t < BP_HT; ++t) {
            uint32_t hi = tile * BP_HT + t;
            if (hi < nh) acc[t] = fe_add<F>(acc[t], fe_dot3<F>(l0, htab[(size_t)b * nh + hi], l1, htab[(size_t)(b + 1) * nh + hi],
                                                               l2, htab[(size_t)(b + 2) * nh + hi]));
        }
    }
    for (; b < b1; ++b) {
        const fe_t l = ltab[(size_t)b * nl + lo];
#pragma unroll
        for (int t = 0; t < BP_HT; ++t) {
            uint32_t hi = tile * BP_HT + t;
            if (hi < nh) acc[t] = fe_add<F>(acc[t], fe_mul<F>(l, htab[(size_t)b * nh + hi]));
        }
    }
    fe_t *out = partial + ((size_t)blockIdx.y * slices + slice) * ((size_t)1 << sh.k);
#pragma unroll
    for (int t = 0; t < BP_HT; ++t) {
        uint32_t hi = tile * BP_HT + t;
        if (hi < nh) out[((size_t)hi << sh.lb) + lo] = acc[t];
    }
}

// out[s][j] (canonical words) = sum over slices of partial[s][slice][j].  With one slice the fold wrote into `out` itself and this converts in place (every lane
// reads its element before it writes it): no __restrict__ here.
template <int F>
__global__ void bpoly_finish_seg_kernel(uint32_t n, uint32_t slices, MsmSegments sg, BpolySegSkip skip, const fe_t *partial, uint32_t *out_words) { mb_wave_prio<1>();
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    uint32_t first, len;
    msm_segment_range(sg, blockIdx.y, sg.n_total, first, len);
    if (bpoly_seg_skipped(skip, len)) return;
    const fe_t *p = partial + (size_t)blockIdx.y * slices * n;
    fe_t acc = p[j];
    for (uint32_t s = 1; s < slices; ++s) acc = fe_add<F>(acc, p[(size_t)s * n + j]);
    acc = fe_from_mont<F>(acc);
    uint4 *o = reinterpret_cast<uint4 *>(out_words + ((size_t)blockIdx.y * n + j) * 8);
    o[0] = make_uint4(acc.v[0], acc.v[1], acc.v[2], acc.v[3]);
    o[1] = make_uint4(acc.v[4], acc.v[5], acc.v[6], acc.v[7]);
}

}  // namespace mb
