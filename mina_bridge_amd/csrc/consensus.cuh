// consensus.cuh -- Samasika chain selection between the bridge's tip and a candidate tip as host/device functions.
//
// The bodies of api_consensus.hip's entry points: the host C-ABI (argument checks there) and the device pre-check of the packed-on-device front end
// (state_pack.cuh pstate_precheck_kernel) compile THIS text, so the two cannot drift.  Specification: the reference's README "Consensus" section (short/long-range
// fork rules, sliding-window density, ring-shift, projected window, relative minimum window density) and its selectSecureChain / selectLongerChain figures.
//
// Written so that a kernel keeps everything in registers: the states are read through their pointers (on the device they point into HBM), no function makes a local
// copy of a window, and the tie-break digests are passed beside the states instead of being copied into them.
#pragma once
#include "fp.cuh"
#include "../../include/mina_verify.h"

namespace mb {

// lexicographic order of two 32-byte strings, as memcmp: < 0, 0, > 0
MB_HD int cs_cmp32(const uint8_t *a, const uint8_t *b) {
    for (int i = 0; i < 32; ++i) { if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1; }
    return 0;
}
MB_HD bool cs_params_ok(const mina_consensus_params *p) {
    return p->sub_windows_per_window != 0 && p->sub_windows_per_window <= MINA_MAX_SUB_WINDOWS && p->slots_per_sub_window != 0;
}
// the ring-shift of "Projected window": how many sub-windows are zeroed (shift) and the relative sub-window of W's most recent one (cur)
MB_HD void cs_ring_shift(const mina_consensus_params *p, const mina_consensus_state *s, uint32_t next_global_slot, uint32_t &shift, uint32_t &cur) {
    const uint32_t n = p->sub_windows_per_window;
    const uint32_t sw_cur = s->curr_global_slot / p->slots_per_sub_window, sw_next = next_global_slot / p->slots_per_sub_window;
    const uint32_t k = sw_next - sw_cur;
    shift = k > 0 ? k - 1 : 0;
    if (shift > n) shift = n;
    cur = sw_cur % n;
}
// W projected to global slot `next`: shift_count = min(max(k - 1, 0), sub_windows_per_window) zero densities, k = subwindow(next) - subwindow(W), starting after W's
// most recent sub-window; k == 0: unchanged; disjoint windows: everything zeroed.  The caller has checked cs_params_ok and next >= curr_global_slot.
MB_HD void cs_project_window(const mina_consensus_params *p, const mina_consensus_state *s, uint32_t next_global_slot, uint32_t *out_window) {
    const uint32_t n = p->sub_windows_per_window;
    for (uint32_t i = 0; i < n; ++i) out_window[i] = s->sub_window_densities[i];
    uint32_t shift, i; cs_ring_shift(p, s, next_global_slot, shift, i);
    while (shift--) { i = (i + 1) % n; out_window[i] = 0; }
}
// density (the sum) of that projected window without storing it: sub-window i is zeroed iff it is one of the `shift` that follow `cur` on the ring
MB_HD uint32_t cs_projected_density(const mina_consensus_params *p, const mina_consensus_state *s, uint32_t next_global_slot) {
    const uint32_t n = p->sub_windows_per_window;
    uint32_t shift, cur; cs_ring_shift(p, s, next_global_slot, shift, cur);
    uint32_t sum = 0;
    for (uint32_t i = 0; i < MINA_MAX_SUB_WINDOWS; ++i) {
        if (i >= n) break;
        const uint32_t after = i > cur ? i - cur - 1 : i + n - cur - 1;      // (i - cur - 1) mod n: sub-windows between `cur` and i on the ring
        if (after >= shift) sum += s->sub_window_densities[i];
    }
    return sum;
}
// "Relative minimum window density": project `a`'s window to the later of the two global slots and take min(a.min_window_density, density(projected window)).
// false: bad parameters.
MB_HD bool cs_relative_min_window_density(const mina_consensus_params *p, const mina_consensus_state *a, const mina_consensus_state *b, uint32_t *out) {
    if (!cs_params_ok(p)) return false;
    const uint32_t max_slot = a->curr_global_slot > b->curr_global_slot ? a->curr_global_slot : b->curr_global_slot;
    const uint32_t d = cs_projected_density(p, a, max_slot);
    *out = d < a->min_window_density ? d : a->min_window_density;
    return true;
}
// "Short-range fork check": same epoch -> same lock_checkpoint in the previous (staking) epoch data; one epoch apart -> the later block's previous-epoch
// lock_checkpoint equals the earlier block's current(next)-epoch one.
MB_HD bool cs_is_short_range(const mina_consensus_state *a, const mina_consensus_state *b) {
    if (a->epoch_count == b->epoch_count) return cs_cmp32(a->staking_lock_checkpoint, b->staking_lock_checkpoint) == 0;
    if (a->epoch_count == b->epoch_count + 1) return cs_cmp32(a->staking_lock_checkpoint, b->next_lock_checkpoint) == 0;
    if (b->epoch_count == a->epoch_count + 1) return cs_cmp32(b->staking_lock_checkpoint, a->next_lock_checkpoint) == 0;
    return false;
}
// the two digests chain selection breaks ties with (both compared lexicographically): hashLastVRF and hashState
struct CsTie { const uint8_t *vrf_hash, *state_hash; };
// selectLongerChain.  true: the candidate is selected; false: the tip is kept.
MB_HD bool cs_select_longer(const mina_consensus_state *tip, const CsTie &tt, const mina_consensus_state *cand, const CsTie &ct) {
    if (tip->blockchain_length < cand->blockchain_length) return true;
    if (tip->blockchain_length == cand->blockchain_length) {
        const int v = cs_cmp32(ct.vrf_hash, tt.vrf_hash);
        if (v > 0) return true;
        if (v == 0 && cs_cmp32(ct.state_hash, tt.state_hash) > 0) return true;
    }
    return false;
}
// selectSecureChain for one candidate: *selected = the candidate replaces the tip.  false: bad parameters (only looked at on the long-range path, as ever).
MB_HD bool cs_select_secure_chain(const mina_consensus_params *p, const mina_consensus_state *tip, const CsTie &tt, const mina_consensus_state *cand, const CsTie &ct,
                                  bool *selected) {
    if (cs_is_short_range(cand, tip)) { *selected = cs_select_longer(tip, tt, cand, ct); return true; }
    uint32_t td = 0, cd = 0;
    if (!cs_relative_min_window_density(p, tip, cand, &td) || !cs_relative_min_window_density(p, cand, tip, &cd)) return false;
    if (cd > td) *selected = true;
    else if (cd == td) *selected = cs_select_longer(tip, tt, cand, ct);
    else *selected = false;
    return true;
}

}  // namespace mb
