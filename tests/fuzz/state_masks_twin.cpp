// state_masks_twin.cpp -- csrc/state_masks.h compiled for the host: prints the rule's answer for EVERY combination of its inputs, one line each
//   <front: -1 absent, else the word> <deny> <sections: bit 0 states, 1 accumulator, 2 ipa> <bits: bit 0 chain, 1 stmt, 2 ipa_each, 3 acc_each> <passed> <ran>
// Reads nothing.  tests/test_state_masks_model.py compares the table with a restatement of the rule.
#include <cstdio>
#include "../../mina_bridge_amd/csrc/state_masks.h"

int main() {
    const uint32_t fronts[8] = {0u, MINA_CHECK_FORMAT, MINA_CHECK_LEDGER, MINA_CHECK_FORMAT | MINA_CHECK_LEDGER, MINA_CHECK_CONSENSUS, MINA_CHECK_FORMAT | MINA_CHECK_CONSENSUS,
                                MINA_CHECK_LEDGER | MINA_CHECK_CONSENSUS, MINA_CHECK_FORMAT | MINA_CHECK_LEDGER | MINA_CHECK_CONSENSUS};
    const uint32_t denies[4] = {0u, MINA_CHECK_FORMAT, MINA_CHECK_KIMCHI, MINA_CHECK_ACCUMULATOR | MINA_CHECK_CHAIN};
    for (int f = -1; f < 8; ++f)
        for (uint32_t deny : denies)
            for (uint32_t sec = 0; sec < 8; ++sec)
                for (uint32_t bits = 0; bits < 16; ++bits) {
                    const mb::StateMasks m = mb::state_masks_of(f >= 0, f >= 0 ? fronts[f] : 0xffffffffu /* must not be read */, deny, sec & 1u, sec & 2u, sec & 4u, bits & 1u, bits & 2u,
                                                                bits & 4u, bits & 8u);
                    printf("%d %u %u %u %u %u\n", f >= 0 ? (int)fronts[f] : -1, deny, sec, bits, m.passed, m.ran);
                }
    return 0;
}
