// bpoly_mfma_seg.cuh -- the matrix-core b_poly fold (bpoly_mfma.cuh) over segments: many folds over ranges [begin, end) of ONE batch in one launch set.
//
// The digit planes are those of bpoly_mfma.cuh, built once per call over the whole batch (batch index contiguous, kpad columns).  A segment is a range of the K
// dimension, so its fold is the same GEMM with the K loop cut down to the 128-byte tiles that cover the range:
//   * the loop starts at begin & ~127 and ends at min(kpad, roundup(end, 128)): every 16-byte load stays aligned and inside the planes;
//   * the first and the last tile may hold columns of neighbouring proofs (and, past the batch, pad columns).  Those bytes of the A operand are cleared in
//     registers between the global load and the LDS store, so their products are zero whatever B holds there.  Whether a tile is such an edge tile is uniform over
//     the block: the tiles inside the range pay one compare;
//   * the accumulators are int32: |C'| <= len * 2^14, so only segments SHORTER than 2^17 may come here (the bound of bpoly_mfma.cuh; run_bpoly_fold_segments in
//     api_sponge.hip classifies on the host, and the kernel clamps the length it reads from the table to the launch's longest segment, which is below 2^17);
//   * which segments run here is a compact list of segment ids (device memory, written by the host that classified them): block (x, y) folds segment
//     ids[first_slot + y] into colsum[y], and the reduce kernel carries colsum[y] into out[ids[first_slot + y]].
// The segment tables are device memory the caller may rewrite while a call is queued (segments.cuh): a range is clamped to the batch, an id to the table, an empty
// range loads nothing and yields zero.  A stale table gives a wrong sum, never an access past the planes, colsum or the output.
//
// The body of the GEMM is restated here and not shared with bpoly_field_gemm_kernel: that kernel's registers and LDS are pinned (tests/test_code_object.py).
#pragma once
#include "bpoly_mfma.cuh"
#include "segments.cuh"

namespace mb {

static constexpr uint32_t BPM_SEG_END = 1u << 17;                 // segments of this length or more overflow an int32 accumulator: VALU kernels
static constexpr size_t BPM_SEG_COLSUM_BUDGET = (size_t)256 << 20;   // bytes of a lane's colsum the segmented fold may ask for: 512 B x 2^k per segment of a pass
// segments per pass at 2^k outputs: as many as the budget holds, one at the least (k = 20: 512 MiB for the one)
static inline uint32_t bpm_seg_per_pass(uint32_t k) { const size_t s = BPM_SEG_COLSUM_BUDGET >> (k + 9); return (uint32_t)(s ? s : 1); }

// bpoly_field_gemm_kernel with the segment on grid.y.  colsum[(y * mtiles * ntiles + mtile * ntiles + ntile) * 64 + column]
__global__ void __launch_bounds__(256)
bpoly_field_gemm_seg_kernel(uint32_t mtiles, uint32_t ntiles, uint32_t kpad, MsmSegments sg, uint32_t nseg, uint32_t n_max, const uint32_t *__restrict__ ids,
                            const int8_t *__restrict__ A, const int8_t *__restrict__ B, unsigned long long *__restrict__ colsum) { mb_wave_prio<1>();
    __shared__ __attribute__((aligned(16))) int8_t tiles[2][2][128 * BPM_ROW];   // stage, A | B, 128 rows
    __shared__ unsigned long long bins[4][4][BPM_COLS];           // wave, tile of the wave, column
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint32_t bmn = (mtiles + 3) / 4, bm = blockIdx.x % bmn, bn = blockIdx.x / bmn;
    const uint32_t mt0 = bm * 4 + (wave & 1u) * 2, nt0 = bn * 4 + (wave >> 1) * 2;       // first of this wave's 2 x 2 tiles
    uint32_t seg = ids[blockIdx.y], first, len;
    seg = seg < nseg ? seg : nseg - 1;
    msm_segment_range(sg, seg, n_max, first, len);
    const uint32_t end = first + len;                            // <= n_total <= kpad
    const uint32_t kb = first & ~(BPM_KT - 1), ke_ = (end + BPM_KT - 1) & ~(BPM_KT - 1), ke = len == 0 ? kb : (ke_ < kpad ? ke_ : kpad);
    for (uint32_t i = lane; i < 4 * BPM_COLS; i += 64) (&bins[wave][0][0])[i] = 0ull;
    bp_v16i acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;
    // loader: thread t fetches rows t/8 + 32 i (i < 4) of the block's 128 A rows and 128 B rows, bytes (t % 8) * 16 .. + 16 of the K tile.
    // Rows past the matrix (nh or nl < 4 tiles) read row 0: their products land in tiles that are never written out.
    const uint32_t lrow = tid >> 3, lcol = (tid & 7u) * 16;
    const int8_t *ga[4], *gb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t ra = bm * 128 + lrow + 32 * i, rb = bn * 128 + lrow + 32 * i;
        ga[i] = A + (size_t)(ra < mtiles * 32 ? ra : 0) * kpad + lcol;
        gb[i] = B + (size_t)(rb < ntiles * 32 ? rb : 0) * kpad + lcol;
    }
    bp_v4i ra4[4], rb4[4];
    auto fetch = [&](uint32_t k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { ra4[i] = *reinterpret_cast<const bp_v4i *>(ga[i] + k0); rb4[i] = *reinterpret_cast<const bp_v4i *>(gb[i] + k0); }
    };
    // the tile at k0 as it goes into LDS: in an edge tile the A bytes of the columns outside [first, end) are cleared (this lane: columns k0 + lcol .. + 16)
    auto stash = [&](int stage, uint32_t k0) {
        if (k0 < first || k0 + BPM_KT > end) {
            const uint32_t c0 = k0 + lcol;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                uint32_t keep = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) { const uint32_t col = c0 + 4 * w + j; keep |= (col >= first && col < end) ? 0xffu << (8 * j) : 0u; }
#pragma unroll
                for (int i = 0; i < 4; ++i) ra4[i][w] &= (int)keep;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<bp_v4i *>(&tiles[stage][0][(lrow + 32 * i) * BPM_ROW + lcol]) = ra4[i];
            *reinterpret_cast<bp_v4i *>(&tiles[stage][1][(lrow + 32 * i) * BPM_ROW + lcol]) = rb4[i];
        }
    };
    // fragment of lane l: row (l & 31) of the MFMA tile, 16 consecutive k at (l >> 5) * 16 of each 32-byte k-step
    const uint32_t fa = ((wave & 1u) * 64 + (lane & 31u)) * BPM_ROW + (lane >> 5) * 16, fb = ((wave >> 1) * 64 + (lane & 31u)) * BPM_ROW + (lane >> 5) * 16;
    if (kb < ke) { fetch(kb); stash(0, kb); }                    // (an empty range loads nothing: kb may be kpad itself)
    __syncthreads();
    int stage = 0;
    for (uint32_t k0 = kb; k0 < ke; k0 += BPM_KT) {
        const bool more = k0 + BPM_KT < ke;
        if (more) fetch(k0 + BPM_KT);                              // global loads of the next tile fly during this tile's MFMAs
        const int8_t *ta = tiles[stage][0], *tb = tiles[stage][1];
#pragma unroll
        for (uint32_t ks = 0; ks < BPM_KT; ks += 32) {
            bp_v4i a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) { a[i] = *reinterpret_cast<const bp_v4i *>(ta + fa + i * 32 * BPM_ROW + ks); b[i] = *reinterpret_cast<const bp_v4i *>(tb + fb + i * 32 * BPM_ROW + ks); }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (more) stash(stage ^ 1, k0 + BPM_KT);
        __syncthreads();
        stage ^= 1;
    }
    const bool m_ok[2] = {mt0 < mtiles, mt0 + 1 < mtiles}, n_ok[2] = {nt0 < ntiles, nt0 + 1 < ntiles};
    // C/D layout: col = lane & 31 (the B row: digit c of lo), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (digit a of hi); bin a + c
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const uint32_t row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), col = lane & 31u;
                atomicAdd(&bins[wave][i * 2 + j][row + col], (unsigned long long)(long long)acc[i][j][r]);
            }
    __syncthreads();
    unsigned long long *cs = colsum + (size_t)blockIdx.y * mtiles * ntiles * BPM_COLS;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
            if (m_ok[i] && n_ok[j]) cs[((size_t)(mt0 + i) * ntiles + (nt0 + j)) * BPM_COLS + lane] = bins[wave][i * 2 + j][lane];
}

// bpoly_colsum_reduce_kernel with the slot on grid.y: colsum[y] -> canonical words at out[ids[y]][(hi << lb) + lo]
template <int F>
__global__ void __launch_bounds__(256)
bpoly_colsum_reduce_seg_kernel(uint32_t nh, uint32_t nl, uint32_t lb, uint32_t nseg, FieldK fk, const uint32_t *__restrict__ ids, const unsigned long long *__restrict__ colsum,
                               uint32_t *__restrict__ out_words) { mb_wave_prio<1>();
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= nh * nl) return;
    uint32_t seg = ids[blockIdx.y];
    seg = seg < nseg ? seg : nseg - 1;
    const uint32_t hi = gid / nl, lo = gid % nl;
    const long long *cs = reinterpret_cast<const long long *>(colsum) + ((size_t)blockIdx.y * nh * nl + gid) * BPM_COLS;      // tile (hi, lo) = tile index gid
    uint32_t limb[17];
#pragma unroll
    for (int i = 0; i < 17; ++i) limb[i] = 0;
    long long carry = 0;
#pragma unroll 1
    for (int k = 0; k < 68; ++k) {                                // 63 columns, then the carry runs out (T < 2^528)
        const long long v = (k < 63 ? cs[k] : 0ll) + carry;
        limb[k >> 2] |= (uint32_t)(v & 0xff) << (8 * (k & 3));
        carry = v >> 8;                                            // arithmetic: the columns are signed, T is not
    }
    fe_t t0, t1, t2 = fe_zero(), one = fe_zero();
    one.v[0] = 1u;
#pragma unroll
    for (int i = 0; i < 8; ++i) { t0.v[i] = limb[i]; t1.v[i] = limb[8 + i]; }
    t2.v[0] = limb[16];
    // T / R = t0 / R + t1 + t2 R  (mod p):  mont(x, 1) = x / R,  mont(x, R^2) = x R
    fe_t r = fe_mul<F>(t0, one);
    r = fe_add<F>(r, fe_mul<F>(fe_mul<F>(t1, fk.r2), one));
    r = fe_add<F>(r, fe_mul<F>(t2, fk.r2));
    r = fe_from_mont<F>(r);
    uint4 *o = reinterpret_cast<uint4 *>(out_words + ((size_t)seg * nh * nl + ((size_t)hi << lb) + lo) * 8);
    o[0] = make_uint4(r.v[0], r.v[1], r.v[2], r.v[3]);
    o[1] = make_uint4(r.v[4], r.v[5], r.v[6], r.v[7]);
}

}  // namespace mb
