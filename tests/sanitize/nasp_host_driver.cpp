// tests/test_nasp_sanitize.py: the library's host-side NA3 / NA4 arithmetic (csrc/kde_host_math.h) under ASan/UBSan; prints
// the threshold's bits and, per sigma, the table length and every weight's bits for the test to compare with the checker
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../kinectdepthmapenhancement_amd/csrc/kde_host_math.h"

int main()
{
    const float t = kde::nasp_acos_threshold();
    uint32_t b;
    memcpy(&b, &t, 4);
    printf("threshold %08x\n", b);
    const float sigmas[] = {10.0f, 50.0f, 0.5f, 0.0f, 1e4f};
    for (float sigma : sigmas) {
        const long long cap = 3 * 255 * 255 + 1;
        std::vector<float> tab((size_t)cap);
        bool zero = false;
        const int n = kde::nasp_weight_table(sigma, cap, tab.data(), &zero);
        printf("table %g %d %d", (double)sigma, n, zero ? 1 : 0);
        for (int i = 0; i < n; i += (n > 4000 ? 97 : 1)) {
            memcpy(&b, &tab[(size_t)i], 4);
            printf(" %d:%08x", i, b);
        }
        printf("\n");
    }
    printf("nasp host driver ok\n");
    return 0;
}
