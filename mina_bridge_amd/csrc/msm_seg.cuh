// msm_seg.cuh -- K1's digit pass over segments: segment s is problem s of the multi-problem pipeline (MsmShape::nprob, bucket sets per problem).  The pipeline's
// problems all have sh.n scalars; here sh.n is the LONGEST segment, problem m reads scalar begin[m] + i and refers to point begin[m] + i of the one base array, and
// the lanes past its own length write no entry.  Only the kernels that cut digits know about segments: everything behind the sort (accumulate, heavy buckets, redo,
// 2-D reduction, finish) sees bucket lists of point references, as before.  These are separate kernels, not a switch inside msm_part_kernel / msm_digits_kernel:
// the existing instantiations compile to what they did.
#pragma once
#include "msm.cuh"
#include "segments.cuh"

namespace mb {

// msm_digits_kernel over segments (the atomic counting sort: partition tables beyond the partitioned sort's limits)
static __global__ void msm_digits_seg_kernel(MsmShape sh, MsmSegments sg, const uint32_t *__restrict__ scalars /* n_total x 8 */,
                                             uint32_t *__restrict__ count, uint32_t *__restrict__ ekey,
                                             uint32_t *__restrict__ eval, uint32_t *__restrict__ eoff) { mb_wave_prio<1>();
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t per_prob = (size_t)sh.n * sh.W;
    if (e >= per_prob * sh.nprob) return;
    const uint32_t m = (uint32_t)(e / per_prob);
    const uint32_t ep = (uint32_t)(e - (size_t)m * per_prob);
    const uint32_t w = ep / sh.n, i = ep % sh.n;
    uint32_t first, len;
    msm_segment_range(sg, m, sh.n, first, len);
    if (i >= len) { ekey[e] = MSM_INVALID; return; }
    uint32_t s[8];
    load_scalar(scalars + (size_t)(first + i) * 8, s);
    uint32_t bucket, ref;
    if (!msm_entry(sh, s, m, w, i, bucket, ref)) { ekey[e] = MSM_INVALID; return; }
    ekey[e] = bucket;
    eval[e] = (first + i) | (ref & 0x80000000u);
    eoff[e] = atomicAdd(&count[bucket], 1u);
}

// msm_part_kernel (K1p-a / K1p-c) over segments: block (m, g) owns scalars g * 256 .. of segment m, all windows
template <bool SCATTER>
static __global__ void __launch_bounds__(1024)
msm_part_seg_kernel(MsmShape sh, SortShape ss, MsmSegments sg, const uint32_t *__restrict__ scalars, uint32_t *__restrict__ gh, uint2 *__restrict__ staging,
                    uint32_t *__restrict__ ekey) { mb_wave_prio<1>();
    __shared__ uint32_t cur[1024];
    const uint32_t tid = threadIdx.x;
    const uint32_t m = blockIdx.x / ss.Gl, g = blockIdx.x - m * ss.Gl;
    uint32_t *ghm = gh + (size_t)m * ss.Pl * ss.Gl + g;
    for (uint32_t j = tid; j < ss.Pl; j += 1024) cur[j] = SCATTER ? ghm[(size_t)j * ss.Gl] : 0u;
    __syncthreads();
    uint32_t first, len;
    msm_segment_range(sg, m, sh.n, first, len);
    const uint32_t i = g * 256 + (tid & 255);                                     // scalar index within the segment
    if (i < len) {
        uint32_t *ek = ekey + (size_t)m * sh.W * sh.n + i;
        if (SCATTER) {
            for (uint32_t w = tid >> 8; w < sh.W; w += 4) {
                const uint32_t key = ek[(size_t)w * sh.n];
                if (key == MSM_INVALID) continue;
                const uint32_t lb = key & 0x7fffffffu;
                const uint32_t pos = atomicAdd(&cur[lb >> ss.fbits], 1u);
                staging[pos] = make_uint2((first + i) | (key & 0x80000000u), lb & ((1u << ss.fbits) - 1u));
            }
        } else {
            uint32_t s[8];
            load_scalar(scalars + (size_t)(first + i) * 8, s);
            for (uint32_t w = tid >> 8; w < sh.W; w += 4) {
                uint32_t bucket, ref;
                if (!msm_entry(sh, s, m, w, i, bucket, ref)) { ek[(size_t)w * sh.n] = MSM_INVALID; continue; }
                const uint32_t lb = bucket - m * ss.SB;
                ek[(size_t)w * sh.n] = lb | (ref & 0x80000000u);
                atomicAdd(&cur[lb >> ss.fbits], 1u);
            }
        }
    }
    if (!SCATTER) {
        __syncthreads();
        for (uint32_t j = tid; j < ss.Pl; j += 1024) ghm[(size_t)j * ss.Gl] = cur[j];
    }
}

}  // namespace mb
