// net_route.h -- which index set the kimchi step of ONE Proof-of-State proof runs against, or that the proof is of the wrong network.  One rule for every entry
// point of the boundary (api_verify.hip: parse_proof_half, state_checks, state_checks_batch); tests/test_net_route_model.py compiles it for the host
// (tests/fuzz/net_route_twin.cpp) and compares it with a restatement over its whole domain.
//
// `flag` is `is_state_proof_from_devnet` of the proof's public input (0 = mainnet, 1 = devnet), as parsed.
//   LEGACY mode (the process holds ONE index pair, in set 0):
//     declared == -1 (no network declared): the flag is not looked at; set 0.
//     declared == n  (mina_verify_set_network): the flag must equal n, else wrong network; set 0.
//     `ready` is not looked at.
//   NETWORK mode (an index pair per network, mina_verify_install_*_net: set n holds network n's):
//     the proof's network is its flag; set `flag` when that set is ready -- it holds what a full configuration needs -- else wrong network.
//     `declared` is not looked at (it is -1 in this mode: a process either declares one network or installs per network).
// A wrong-network proof fails the kimchi step (the step ran and did not pass); its other checks keep their own bits, and no other proof's verdict is affected.
#pragma once

namespace mb {

enum NetMode : int { NET_LEGACY = 0, NET_NETWORK = 1 };
struct NetRoute { int set; bool reject; };      // set: 0 | 1, meaningful where !reject (0 otherwise)

inline NetRoute net_route(int mode, int declared, const bool ready[2], int flag) {
    const int f = flag ? 1 : 0;
    if (mode == NET_NETWORK) return ready[f] ? NetRoute{f, false} : NetRoute{0, true};
    if (declared < 0) return NetRoute{0, false};
    return f == declared ? NetRoute{0, false} : NetRoute{0, true};
}

// MINA_VERIFY_MIXED_NETWORK_JOB: may ONE pass (one job per chunk, the index set chosen per proof on the GPU: ctx.h StateJobPlan::d_net) serve the proofs of both
// networks?  Iff the flag is set, the process is in network mode, both networks are ready, and the two pairs agree on what a job's shape depends on: the wrap
// domain (k[n] = log2 of network n's) and whether the step program looks at a proof's features.  Otherwise the sequential passes run and nothing differs.
// tests/test_mixed_route_model.py walks it over its whole domain (tests/fuzz/mixed_route_twin.cpp).
inline bool mixed_pass_allowed(int mode, const bool ready[2], const unsigned k[2], const bool feature_aware[2], bool flag_set) {
    return flag_set && mode == NET_NETWORK && ready[0] && ready[1] && k[0] == k[1] && feature_aware[0] == feature_aware[1];
}

}  // namespace mb
