// Stand-alone driver of cerberus_amd/csrc/conv_plan.h for tests/test_conv_plan_host.py: no HIP, no library.  One query per line of standard input,
//   conv_algo ks stride cin cout ho wo wino mode planar train_packed  has_resid packed_items site
// and one answer per line: the kernel's name and the profile family.
#include <cstdio>

#include "../../cerberus_amd/csrc/conv_plan.h"

int main() {
    static const char* const names[] = {"igemm", "igemm_planar", "wino2", "wino4", "wino4b", "wino4p", "none"};
    int algo, ks, stride, cin, cout, ho, wo, wino, mode, planar, train, resid, packed, site;
    while (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d", &algo, &ks, &stride, &cin, &cout, &ho, &wo, &wino, &mode, &planar, &train, &resid, &packed, &site) == 14) {
        const ConvLayer l{algo, ks, stride, cin, cout, ho, wo, wino != 0, mode, planar != 0, train != 0};
        const ConvKernel k = conv_plan(l);
        printf("%s %s\n", names[k], k == CONV_NONE ? "-" : conv_family(k, l, resid != 0, packed != 0, site).c_str());
    }
    return 0;
}
