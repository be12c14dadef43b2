// mixed_route_twin.cpp -- csrc/net_route.h mixed_pass_allowed compiled for the host: prints the rule's answer over its WHOLE domain (wrap domains 14 .. 16), one line each
//   <mode: 0 legacy, 1 network> <ready: bit 0 set 0, bit 1 set 1> <k0> <k1> <feature_aware: bit 0 set 0, bit 1 set 1> <flag set> <allowed>
// Reads nothing.  tests/test_mixed_route_model.py compares the table with a restatement of the rule.
#include <cstdio>
#include "../../mina_bridge_amd/csrc/net_route.h"

int main() {
    for (int mode = 0; mode < 2; ++mode)
        for (int r = 0; r < 4; ++r)
            for (unsigned k0 = 14; k0 < 17; ++k0)
                for (unsigned k1 = 14; k1 < 17; ++k1)
                    for (int fa = 0; fa < 4; ++fa)
                        for (int flag = 0; flag < 2; ++flag) {
                            const bool ready[2] = {(r & 1) != 0, (r & 2) != 0}, aware[2] = {(fa & 1) != 0, (fa & 2) != 0};
                            const unsigned k[2] = {k0, k1};
                            printf("%d %d %u %u %d %d %d\n", mode, r, k0, k1, fa, flag, mb::mixed_pass_allowed(mode, ready, k, aware, flag != 0) ? 1 : 0);
                        }
    return 0;
}
