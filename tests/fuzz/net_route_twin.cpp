// net_route_twin.cpp -- csrc/net_route.h compiled for the host: prints the rule's answer over its WHOLE domain, one line each
//   <mode: 0 legacy, 1 network> <declared: -1 | 0 | 1> <ready: bit 0 set 0, bit 1 set 1> <flag> <set> <reject>
// Reads nothing.  tests/test_net_route_model.py compares the table with a restatement of the rule.
#include <cstdio>
#include "../../mina_bridge_amd/csrc/net_route.h"

int main() {
    for (int mode = 0; mode < 2; ++mode)
        for (int declared = -1; declared < 2; ++declared)
            for (int r = 0; r < 4; ++r)
                for (int flag = 0; flag < 2; ++flag) {
                    const bool ready[2] = {(r & 1) != 0, (r & 2) != 0};
                    const mb::NetRoute rt = mb::net_route(mode, declared, ready, flag);
                    printf("%d %d %d %d %d %d\n", mode, declared, r, flag, rt.set, rt.reject ? 1 : 0);
                }
    return 0;
}
