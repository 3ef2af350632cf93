// The refusals of pfb_chan_average (csrc/stokes.hip) as a stand-alone host program, for a run under the host's
// AddressSanitizer / UBSan: every call below must come back with its status before any launch, so the program needs no
// GPU.  The pointers are host memory of the right alignment; nothing dereferences them.
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Ipfb_clean_amd/csrc \
//         pfb_clean_amd/csrc/stokes.hip tools/chanavg_refusals_main.cpp -o chanavg_refusals && ./chanavg_refusals
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/pfb_hip.h"

namespace pfb {
static char g_msg[512];
// what fftconv.hip defines in the library
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
    va_end(ap);
}
}  // namespace pfb

static int failures = 0;
static void expect(const char* what, int got, int want) {
    if (got != want) {
        ++failures;
        printf("FAIL %s: status %d, expected %d (%s)\n", what, got, want, pfb::g_msg);
    }
}

int main() {
    alignas(16) static double buf[64];
    void* p = buf;
    unsigned char* b = reinterpret_cast<unsigned char*>(buf);
    struct A {
        int dtype = PFB_F64, nprod = 1;
        const void* vis = nullptr;
        const void* wgt = nullptr;
        const unsigned char* mask = nullptr;
        size_t nrow = 2;
        int nchan = 3, n = 2;
        void* viso = nullptr;
        void* wgto = nullptr;
        unsigned char* masko = nullptr;
        double* wsum = nullptr;
        double* work = nullptr;
    };
    auto alone = [&](A a) {
        return pfb_chan_average(a.dtype, a.nprod, a.vis, a.wgt, a.mask, a.nrow, a.nchan, a.n, a.viso, a.wgto, a.masko, a.wsum,
                                a.work, nullptr);
    };
    A h;
    h.vis = p; h.wgt = p; h.mask = b; h.viso = p; h.wgto = p; h.masko = b; h.wsum = buf; h.work = buf;
    A a;
    a = h; a.n = 0;                    expect("alone n = 0", alone(a), PFB_ERR_INVALID);
    a = h; a.n = -1;                   expect("alone n < 0", alone(a), PFB_ERR_INVALID);
    a = h; a.nprod = 0;                expect("alone nprod = 0", alone(a), PFB_ERR_INVALID);
    a = h; a.nprod = 5;                expect("alone nprod = 5", alone(a), PFB_ERR_INVALID);
    a = h; a.dtype = -1;               expect("alone dtype", alone(a), PFB_ERR_INVALID);
    a = h; a.vis = nullptr;            expect("alone null vis", alone(a), PFB_ERR_INVALID);
    a = h; a.wgt = nullptr;            expect("alone null wgt", alone(a), PFB_ERR_INVALID);
    a = h; a.mask = nullptr;           expect("alone null mask", alone(a), PFB_ERR_INVALID);
    a = h; a.viso = nullptr;           expect("alone null viso", alone(a), PFB_ERR_INVALID);
    a = h; a.wgto = nullptr;           expect("alone null wgto", alone(a), PFB_ERR_INVALID);
    a = h; a.masko = nullptr;          expect("alone null masko", alone(a), PFB_ERR_INVALID);
    a = h; a.wsum = nullptr;           expect("alone null wsum", alone(a), PFB_ERR_INVALID);
    a = h; a.work = nullptr;           expect("alone null work", alone(a), PFB_ERR_INVALID);
    a = h; a.vis = b + 8;              expect("alone misaligned vis", alone(a), PFB_ERR_INVALID);
    a = h; a.wgto = b + 4;             expect("alone misaligned wgto", alone(a), PFB_ERR_INVALID);
    a = h; a.nrow = 0;                 expect("alone nrow = 0", alone(a), PFB_ERR_UNSUPPORTED);
    a = h; a.nrow = (size_t)1 << 31;   expect("alone nrow = 2^31", alone(a), PFB_ERR_UNSUPPORTED);
    a = h; a.nchan = 0;                expect("alone nchan = 0", alone(a), PFB_ERR_UNSUPPORTED);
    a = h; a.nchan = -1;               expect("alone nchan < 0", alone(a), PFB_ERR_UNSUPPORTED);
    printf("%s: %d failures\n", failures ? "FAILED" : "all refusals as stated", failures);
    return failures ? 1 : 0;
}
