// api_consensus.hip -- Samasika chain selection between the bridge's tip and a candidate tip, host C++.
//
// Follows the reference's own specification, which is in-tree prose + figures:
//   /root/reference/README.md:619-735  (short/long-range fork rules, decentralized checkpointing, sliding-window density,
//                                       ring-shift, projected window, relative minimum window density)
//   img/consensus07.png  selectSecureChain      img/consensus08.png  selectLongerChain     img/consensus03.png  special cases
// README.md:290-294 says the verifier runs this between `candidate_tip` and `bridge_tip` before the Pickles check.
// The fields come from MinaStateProtocolStateValueStableV2.body.consensus_state (un-vendored type; the binprot parser
// is row 8f-2), so the caller passes them pre-extracted.  The logic itself is consensus.cuh (host and device); these are the host entry points with their argument checks.
#include <cstring>

#include "ctx.h"
#include "consensus.cuh"

// README.md "Projected window" (consensus.cuh cs_project_window)
extern "C" int mina_consensus_project_window(const mina_consensus_params *p, const mina_consensus_state *s, uint32_t next_global_slot,
                                             uint32_t *out_window /* sub_windows_per_window */) {
    if (!p || !s || !out_window) return fail(MINA_ERR_ARG, "null argument");
    if (!mb::cs_params_ok(p)) return fail(MINA_ERR_ARG, "bad consensus parameters");
    if (next_global_slot < s->curr_global_slot) return fail(MINA_ERR_ARG, "cannot project a window into the past");
    mb::cs_project_window(p, s, next_global_slot, out_window);
    return MINA_OK;
}

// README.md "Relative minimum window density" (cs_relative_min_window_density)
extern "C" int mina_consensus_relative_min_window_density(const mina_consensus_params *p, const mina_consensus_state *a,
                                                          const mina_consensus_state *b, uint32_t *out) {
    if (!p || !a || !b || !out) return fail(MINA_ERR_ARG, "null argument");
    if (!mb::cs_relative_min_window_density(p, a, b, out)) return fail(MINA_ERR_ARG, "bad consensus parameters");
    return MINA_OK;
}

// README.md "Short-range fork check" (cs_is_short_range)
extern "C" int mina_consensus_is_short_range(const mina_consensus_state *a, const mina_consensus_state *b) {
    if (!a || !b) return 0;
    return mb::cs_is_short_range(a, b) ? 1 : 0;
}

// img/consensus07.png for one candidate: *candidate_selected = 1 if the candidate replaces the tip (cs_select_secure_chain, cs_select_longer).
extern "C" int mina_consensus_select_secure_chain(const mina_consensus_params *p, const mina_consensus_state *tip,
                                                  const mina_consensus_state *candidate, int *candidate_selected) {
    if (!p || !tip || !candidate || !candidate_selected) return fail(MINA_ERR_ARG, "null argument");
    bool sel = false;
    if (!mb::cs_select_secure_chain(p, tip, mb::CsTie{tip->last_vrf_output_hash, tip->state_hash}, candidate, mb::CsTie{candidate->last_vrf_output_hash, candidate->state_hash}, &sel))
        return fail(MINA_ERR_ARG, "bad consensus parameters");
    *candidate_selected = sel ? 1 : 0;
    return MINA_OK;
}
