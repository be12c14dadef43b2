// state_masks.h -- the `passed` / `ran` masks of ONE Proof-of-State proof, composed from what a job knows about it.  One rule for the masks kernel (api_state.hip
// state_job_masks_kernel) and for the host: it follows the single-proof diagnostic form (api_verify.hip state_checks) line by line, and
// tests/test_state_masks_model.py compiles it for the host and compares it with a restatement over every combination of its inputs.
//
//   ran = FORMAT.
//   If `front` is present and lacks FORMAT, or `deny` has FORMAT: passed = 0, nothing else is in `ran`, and the proof is done.
//   Otherwise passed = FORMAT.
//   With `front` present: ran |= LEDGER | CONSENSUS and passed |= front & (LEDGER | CONSENSUS).  Without it, neither bit runs.
//   with_states:      ran |= CHAIN;       passed iff `chain`.
//   with_accumulator: ran |= ACCUMULATOR; passed iff `acc_each`.
//   with_ipa:         ran |= KIMCHI;      passed iff `stmt && ipa_each`.
//   Finally passed &= ~deny.  `ran` is not touched by `deny`.
#pragma once
#include <stdint.h>
#include "../../include/mina_verify.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MB_MASKS_HD __host__ __device__
#else
#define MB_MASKS_HD
#endif

namespace mb {

struct StateMasks { uint32_t passed, ran; };

// front: the MINA_CHECK_FORMAT | _LEDGER | _CONSENSUS bits that passed (mina_state_frontend_dev's d_masks), read only where have_front; deny: MINA_CHECK_* bits the
// caller has decided fail (0 = none); with_*: the job's section flags; chain: all 17 hashes equal the expected ones and states 1..15 name their predecessor (the
// job's `precheck` byte is not part of it); stmt: the Pickles statement is well-formed; ipa_each / acc_each: not a culprit of the opening / accumulator leg.
MB_MASKS_HD inline StateMasks state_masks_of(bool have_front, uint32_t front, uint32_t deny, bool with_states, bool with_accumulator, bool with_ipa, bool chain, bool stmt,
                                             bool ipa_each, bool acc_each) {
    StateMasks m{0u, MINA_CHECK_FORMAT};
    if ((have_front && !(front & MINA_CHECK_FORMAT)) || (deny & MINA_CHECK_FORMAT)) return m;
    m.passed = MINA_CHECK_FORMAT;
    if (have_front) { m.ran |= MINA_CHECK_LEDGER | MINA_CHECK_CONSENSUS; m.passed |= front & (MINA_CHECK_LEDGER | MINA_CHECK_CONSENSUS); }
    if (with_states) { m.ran |= MINA_CHECK_CHAIN; if (chain) m.passed |= MINA_CHECK_CHAIN; }
    if (with_accumulator) { m.ran |= MINA_CHECK_ACCUMULATOR; if (acc_each) m.passed |= MINA_CHECK_ACCUMULATOR; }
    if (with_ipa) { m.ran |= MINA_CHECK_KIMCHI; if (stmt && ipa_each) m.passed |= MINA_CHECK_KIMCHI; }
    m.passed &= ~deny;
    return m;
}

}  // namespace mb
