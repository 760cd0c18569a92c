// The host helpers of topowx_amd/qa/twx_qa_common.h as a program of its own (tests/test_qa_common_host.py): qa_fail in its
// four cases, qa_days_from_civil and qa_leap on the dates given as arguments.  It makes no call that needs a device.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "twx_qa_common.h"

// a function with errbuf / errlen in scope, as every user of QACHK is
static int through_the_macro(hipError_t e, char *errbuf, int errlen)
{
    QACHK(e);
    return 0;
}

int main(int argc, char **argv)
{
    char buf[96];
    int rc = qa_fail(buf, (int)sizeof buf, "twxqa_demo: need n >= 1");
    printf("plain %d [%s]\n", rc, buf);
    printf("errstr [%s]\n", hipGetErrorString(hipErrorOutOfMemory));
    rc = qa_fail(buf, (int)sizeof buf, "hipMalloc(&p, n)", hipErrorOutOfMemory);
    printf("hip %d [%s]\n", rc, buf);
    rc = through_the_macro(hipErrorOutOfMemory, buf, (int)sizeof buf);
    printf("macro %d [%s]\n", rc, buf);
    rc = through_the_macro(hipSuccess, buf, (int)sizeof buf);
    printf("macro_ok %d\n", rc);

    char guard[16];                                              // 4 guard bytes, a buffer of 8, 4 guard bytes
    memset(guard, '#', sizeof guard);
    rc = qa_fail(guard + 4, 8, "0123456789abcdef");
    const bool intact = memcmp(guard, "####", 4) == 0 && memcmp(guard + 12, "####", 4) == 0;
    printf("short %d [%s] len %d guards %d\n", rc, guard + 4, (int)strlen(guard + 4), intact ? 1 : 0);

    strcpy(buf, "keep");
    const int rc_null = qa_fail(nullptr, 64, "x"), rc_zero = qa_fail(buf, 0, "x"), rc_neg = qa_fail(buf, -1, "x");
    printf("none %d %d %d [%s]\n", rc_null, rc_zero, rc_neg, buf);

    for (int i = 1; i + 2 < argc; i += 3) {
        const int y = atoi(argv[i]), m = atoi(argv[i + 1]), d = atoi(argv[i + 2]);
        printf("date %d %d %d %lld %d\n", y, m, d, (long long)qa_days_from_civil(y, m, d), qa_leap(y) ? 1 : 0);
    }
    return 0;
}
