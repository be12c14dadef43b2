// state_dedup.cuh -- the opt-in deduplication of a job's protocol-state records (mina_ctx_set_state_dedup; api_state.hip pstate_hash_dedup_dev).
//
// Records i and j are THE SAME iff their clamped field counts agree and their first 1 + n_body_fields slots are byte-identical; rep[i] is the smallest index whose
// record is the same as record i.  A 128-bit fingerprint only chooses where a record looks in an open-addressed table; EQUALITY OF THE RECORDS decides whether it
// joins the class it finds there, so no two different records ever share a result, whatever the fingerprint does (fingerprint_bits cuts it to a few bits to test that).
//
// The table (16 B per entry, a power of two >= 2 n entries: at most half full, set to all-ones before every use): `word` = (41-bit tag of the fingerprint << 22) |
// owner, claimed ONCE by a 64-bit atomicCAS; the owner's record is what later arrivals are compared with -- it never changes, so every class of equal records ends
// in exactly one entry whatever order the lanes ran in --; `min` = the smallest index that joined the entry (atomicMin).  Inside pstate_dedup_group_kernel all
// table traffic is device-scope atomics (a plain store is not seen across XCDs); the records themselves are read-only input.  pstate_dedup_rep_kernel reads `min`
// behind the kernel boundary.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mb {

struct DedupSlot { unsigned long long word; uint32_t min; uint32_t pad; };
static constexpr unsigned long long DEDUP_EMPTY = ~0ull;
static constexpr uint32_t DEDUP_OWNER_BITS = 22;                     // n <= 2^22 records per call
static constexpr uint32_t DEDUP_NO_SLOT = 0xffffffffu;
static constexpr uint32_t DEDUP_SUB = 16;                            // lanes per record: 16 x 16 B = 256 contiguous bytes per load, 8 loads cover the 2 KiB
static constexpr uint32_t DEDUP_CHUNKS = MINA_PSTATE_SLOTS * 2;      // 16-byte pieces of a record
static constexpr uint32_t DEDUP_PER_LANE = DEDUP_CHUNKS / DEDUP_SUB;
static constexpr uint32_t DEDUP_SCAN_ITEMS = 4, DEDUP_SCAN_BLOCK = 256, DEDUP_SCAN_TILE = DEDUP_SCAN_ITEMS * DEDUP_SCAN_BLOCK;

__device__ __forceinline__ unsigned long long dedup_fmix(unsigned long long x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33; return x;
}
__device__ __forceinline__ unsigned long long dedup_bcast64(unsigned long long v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long dedup_xor16(unsigned long long v) {          // xor over the 16 lanes of a record (DPP row moves: no LDS)
#pragma unroll
    for (int d = 1; d < (int)DEDUP_SUB; d <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
        v ^= ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

// One sub-wave of 16 lanes per record.  The record is read ONCE (16 B per lane per load, the loads of a sub-wave contiguous), mixed into a 128-bit fingerprint of its
// used slots and its field count, and kept in registers for the comparisons.  Then the sub-wave walks the table from the fingerprint's slot: an empty entry is claimed,
// an entry with its tag whose owner's record EQUALS this one is joined, anything else (another tag, or the same tag and a different record: a collision, counted) sends
// it to the next entry.  At most `tmask + 1` probes; the table is at most half full, so an empty entry is always met first.  slot_of[i] = the entry record i joined.
__global__ void __launch_bounds__(256)
pstate_dedup_group_kernel(uint32_t n, uint32_t tmask, uint32_t fingerprint_bits, const uint32_t *__restrict__ records, const uint32_t *__restrict__ nfields,
                          DedupSlot *table, uint32_t *__restrict__ slot_of, uint32_t *counts /* [1] += collisions */) {
    const uint32_t lane = threadIdx.x & 63u, l = lane & (DEDUP_SUB - 1), sub = lane / DEDUP_SUB;
    const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) / DEDUP_SUB;
    const bool live = i < n;
    const uint32_t ii = live ? i : 0;                                  // dead sub-waves shadow record 0 (whole waves run the cross-lane moves)
    const uint4 *__restrict__ r4 = reinterpret_cast<const uint4 *>(records);
    uint32_t nf = nfields[ii]; if (nf > MINA_PSTATE_SLOTS - 1) nf = MINA_PSTATE_SLOTS - 1;
    const uint32_t used = 2 * (1 + nf);                                // 16-byte pieces that count
    uint4 mine[DEDUP_PER_LANE];
#pragma unroll
    for (uint32_t k = 0; k < DEDUP_PER_LANE; ++k) {
        const uint32_t ch = l + DEDUP_SUB * k;
        mine[k] = make_uint4(0, 0, 0, 0);
        if (ch < used) mine[k] = r4[(size_t)ii * DEDUP_CHUNKS + ch];
    }
    // fingerprint: each lane chains its pieces (their order = their position), the lanes' results are xor-ed; not a security boundary
    unsigned long long a = 0x9e3779b97f4a7c15ull * (l + 1) + nf, b = 0xc2b2ae3d27d4eb4full ^ ((unsigned long long)l << 32);
#pragma unroll
    for (uint32_t k = 0; k < DEDUP_PER_LANE; ++k) {
        const unsigned long long k0 = ((unsigned long long)mine[k].y << 32) | mine[k].x, k1 = ((unsigned long long)mine[k].w << 32) | mine[k].z;
        a = (a ^ k0) * 0x9e3779b97f4a7c15ull; a ^= a >> 32;
        b = (b ^ k1 ^ a) * 0xc2b2ae3d27d4eb4full; b ^= b >> 29;
        a += b;
    }
    a = dedup_xor16(dedup_fmix(a)); b = dedup_xor16(dedup_fmix(b + a));
    a = dedup_fmix(a + nf); b = dedup_fmix(b ^ a);
    if (fingerprint_bits) { a &= (1ull << fingerprint_bits) - 1; b = dedup_fmix(a); }      // the test mode: both the tag and the first slot follow the cut fingerprint
    const unsigned long long tag = a & ((1ull << 41) - 1);
    const unsigned long long mine_word = (tag << DEDUP_OWNER_BITS) | i;
    uint32_t slot = (uint32_t)b & tmask, probes = 0, joined = DEDUP_NO_SLOT, ncoll = 0;
    bool done = !live;
    while (__any(!done)) {                                             // wave-uniform loop: the cross-lane moves below run with every lane of the wave present
        unsigned long long w = 0;
        if (!done && l == 0) {
            w = __hip_atomic_load(&table[slot].word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (w == DEDUP_EMPTY) { const unsigned long long old = atomicCAS(&table[slot].word, DEDUP_EMPTY, mine_word); w = old == DEDUP_EMPTY ? mine_word : old; }
        }
        w = dedup_bcast64(w, (int)(lane & ~(DEDUP_SUB - 1)));
        const bool cand = !done && (w >> DEDUP_OWNER_BITS) == tag;
        const uint32_t owner = (uint32_t)w & ((1u << DEDUP_OWNER_BITS) - 1);
        bool differ = false;
        if (cand && owner != i && owner < n) {                         // (owner < n always holds: only this kernel writes the words)
            uint32_t nfo = nfields[owner]; if (nfo > MINA_PSTATE_SLOTS - 1) nfo = MINA_PSTATE_SLOTS - 1;
            differ = nfo != nf;
            if (!differ) {
#pragma unroll
                for (uint32_t k = 0; k < DEDUP_PER_LANE; ++k) {
                    const uint32_t ch = l + DEDUP_SUB * k;
                    if (ch < used) { const uint4 o = r4[(size_t)owner * DEDUP_CHUNKS + ch]; differ |= o.x != mine[k].x || o.y != mine[k].y || o.z != mine[k].z || o.w != mine[k].w; }
                }
            }
        }
        const unsigned long long bal = __ballot(differ);
        const bool other = ((bal >> (sub * DEDUP_SUB)) & 0xffffull) != 0;
        if (cand) {
            if (!other) { if (l == 0) atomicMin(&table[slot].min, i); joined = slot; done = true; }
            else if (l == 0) ++ncoll;
        }
        if (!done) { slot = (slot + 1) & tmask; if (++probes > tmask) done = true; }      // unreachable with a half-full table; such a record stands for itself
    }
    if (live && l == 0) slot_of[i] = joined;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) ncoll += (uint32_t)__shfl_xor((int)ncoll, d, 64);
    if (lane == 0 && ncoll) atomicAdd(&counts[1], ncoll);             // one atomic per wave
}

// sum of `v` over the workgroup (DEDUP_SCAN_BLOCK threads) and its exclusive prefix per thread
__device__ __forceinline__ uint32_t dedup_block_scan(uint32_t v, uint32_t &total) {
    __shared__ uint32_t wsum[DEDUP_SCAN_BLOCK / 64];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)inc, d, 64); if (lane >= (uint32_t)d) inc += t; }
    if (lane == 63u) wsum[wv] = inc;
    __syncthreads();
    uint32_t before = 0; total = 0;
#pragma unroll
    for (uint32_t q = 0; q < DEDUP_SCAN_BLOCK / 64; ++q) { const uint32_t s = wsum[q]; if (q < wv) before += s; total += s; }
    __syncthreads();
    return before + inc - v;
}

// behind the kernel boundary: rep[i] = the smallest index of record i's entry (in place over slot_of), and the number of representatives per tile of DEDUP_SCAN_TILE records
__global__ void __launch_bounds__(DEDUP_SCAN_BLOCK)
pstate_dedup_rep_kernel(uint32_t n, const DedupSlot *__restrict__ table, uint32_t *__restrict__ rep, uint32_t *__restrict__ tile_count) {
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t q = 0; q < DEDUP_SCAN_ITEMS; ++q) {
        const uint32_t i = blockIdx.x * DEDUP_SCAN_TILE + threadIdx.x * DEDUP_SCAN_ITEMS + q;
        if (i < n) { const uint32_t s = rep[i]; const uint32_t r = s == DEDUP_NO_SLOT ? i : table[s].min; rep[i] = r; mine += r == i; }
    }
    uint32_t total; (void)dedup_block_scan(mine, total);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

// one workgroup: tile counts -> their exclusive prefix (in place); counts[0] = the number of distinct records; the context's running totals
__global__ void __launch_bounds__(DEDUP_SCAN_BLOCK)
pstate_dedup_scan_kernel(uint32_t ntiles, uint32_t *__restrict__ tile_count, uint32_t *counts, unsigned long long *totals /* {distinct, collisions} or null */) {
    const uint32_t per = (ntiles + DEDUP_SCAN_BLOCK - 1) / DEDUP_SCAN_BLOCK, lo = threadIdx.x * per, hi = min(ntiles, lo + per);
    uint32_t mine = 0;
    for (uint32_t t = lo; t < hi; ++t) mine += tile_count[t];
    uint32_t total; uint32_t run = dedup_block_scan(mine, total);
    for (uint32_t t = lo; t < hi; ++t) { const uint32_t v = tile_count[t]; tile_count[t] = run; run += v; }
    if (threadIdx.x == 0) {
        counts[0] = total;
        if (totals) { atomicAdd(&totals[0], (unsigned long long)total); atomicAdd(&totals[1], (unsigned long long)counts[1]); }
    }
}

// uniq[] = the representatives in ascending order (tile_start: the exclusive prefix pstate_dedup_scan_kernel left)
__global__ void __launch_bounds__(DEDUP_SCAN_BLOCK)
pstate_dedup_compact_kernel(uint32_t n, const uint32_t *__restrict__ rep, const uint32_t *__restrict__ tile_start, uint32_t *__restrict__ uniq) {
    const uint32_t base = blockIdx.x * DEDUP_SCAN_TILE + threadIdx.x * DEDUP_SCAN_ITEMS;
    bool is[DEDUP_SCAN_ITEMS]; uint32_t mine = 0;
#pragma unroll
    for (uint32_t q = 0; q < DEDUP_SCAN_ITEMS; ++q) { const uint32_t i = base + q; is[q] = i < n && rep[i] == i; mine += is[q]; }
    uint32_t total; uint32_t at = tile_start[blockIdx.x] + dedup_block_scan(mine, total);
#pragma unroll
    for (uint32_t q = 0; q < DEDUP_SCAN_ITEMS; ++q) if (is[q]) uniq[at++] = base + q;
}

// The hash kernels wrote every representative's hash at the representative's own place: hashes[i] = hashes[rep[i]] for the other records (and the body hashes where
// asked for).  Two lanes per record, 16 B each; this launch reads representatives' entries and writes the others' only.
__global__ void __launch_bounds__(256)
pstate_dedup_scatter_kernel(uint32_t n, const uint32_t *__restrict__ rep, uint32_t *hashes, uint32_t *bodies /* or null */) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, i = t >> 1, half = t & 1u;
    if (i >= n) return;
    const uint32_t r = rep[i];
    if (r == i) return;
    reinterpret_cast<uint4 *>(hashes)[(size_t)i * 2 + half] = reinterpret_cast<const uint4 *>(hashes)[(size_t)r * 2 + half];
    if (bodies) reinterpret_cast<uint4 *>(bodies)[(size_t)i * 2 + half] = reinterpret_cast<const uint4 *>(bodies)[(size_t)r * 2 + half];
}

}  // namespace mb
