// entry.hpp -- the host side of a C entry point of the visibility-side files (wgrid.hip, imweight.hip, stokes.hip,
// visconcat.hip; DESIGN 4.10, "The entry layer").  An entry point reads top to bottom: check() on its type code and
// pointers, its size checks, its memset, then one launch from a by_type (and by_int) lambda; a sum ends in final_sum.
// A new one needs nothing else.  cgvec.hip, wavelet.hip and hessparam.hip take final_sum from here.  Templates and
// inline functions only, no state.
#pragma once
#include "common.hpp"
#include <type_traits>

namespace pfb {

typedef unsigned char u8;

constexpr double C_LIGHT = 299792458.0;
constexpr int ENTRY_BLOCK = 256;          // threads per workgroup of every kernel launched from here
static_assert(ENTRY_BLOCK == RED_BLOCK, "emit_partials reduces RED_BLOCK threads");

__device__ __forceinline__ void atomic_add(float* p, float v) { unsafeAtomicAdd(p, v); }
__device__ __forceinline__ void atomic_add(double* p, double v) { unsafeAtomicAdd(p, v); }

// ------------------------------------------------------------------------------------------------------- dispatch
inline size_t esize(int dtype) { return dtype == PFB_F32 ? 4 : 8; }
// f(float{}) or f(double{}): the data type (checked before)
template <typename F>
inline int by_type(int dtype, F&& f) { return dtype == PFB_F32 ? f(float{}) : f(double{}); }
// f(std::integral_constant<int, K>{}) for the K of FIRST, FIRST + STEP, .., LAST that equals v (anything else: LAST; the
// range is checked before): one instantiation per value
template <int FIRST, int LAST, int STEP = 1, typename F>
inline int by_int(int v, F&& f) {
    static_assert(FIRST <= LAST && (LAST - FIRST) % STEP == 0, "LAST is one of the values");
    if constexpr (FIRST < LAST) {
        if (v != FIRST) return by_int<FIRST + STEP, LAST, STEP>(v, f);
    }
    return f(std::integral_constant<int, FIRST>{});
}

// --------------------------------------------------------------------------------------------------------- launch
// a void pointer of the C ABI becomes the kernel parameter it is passed for; every other argument goes as it is
template <typename P, typename A>
inline P arg(A a) {
    if constexpr (std::is_void_v<std::remove_pointer_t<A>>) return static_cast<P>(a);
    else return a;
}
inline unsigned blocks(size_t n) { return (unsigned)((n + ENTRY_BLOCK - 1) / ENTRY_BLOCK); }
// `kernel` on `groups` workgroups, on the stream: the strided streaming kernels
template <typename... P, typename... A>
inline int launch_groups(void (*kernel)(P...), size_t groups, void* stream, A... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)groups), dim3(ENTRY_BLOCK), 0, as_stream(stream), arg<P>(args)...);
    PFB_HIP_CHECK(hipGetLastError());
    return PFB_OK;
}
// `kernel` with a lane per element of n
template <typename... P, typename... A>
inline int launch(void (*kernel)(P...), size_t n, void* stream, A... args) {
    return launch_groups(kernel, blocks(n), stream, args...);
}
// out[0 .. nq) = the sums of the partials that a kernel of G workgroups left in ws (emit_partials), in a fixed order.  A
// template, so that only the translation units that call it emit k_final_sum
template <int BLOCK = RED_BLOCK>
inline int final_sum(const double* ws, int G, int nq, double* out, void* stream) {
    hipLaunchKernelGGL(k_final_sum<BLOCK>, dim3(1), dim3(BLOCK), 0, as_stream(stream), ws, G, nq, out);
    PFB_HIP_CHECK(hipGetLastError());
    return PFB_OK;
}

// --------------------------------------------------------------------------------------------------------- checks
// the alignment of a pointer argument: `elems` elements of the entry point's type plus `bytes`.  REAL and CPLX are of
// that type; bytes(n) states the width of a kernel's vector loads
struct Align { size_t elems, bytes; };
constexpr Align REAL{1, 0}, CPLX{2, 0}, F64{0, 8}, I64{0, 8}, I32{0, 4}, U8{0, 1};
constexpr Align bytes(size_t n) { return {0, n}; }
struct Array { const void* ptr; Align align; bool optional = false; };

// the type code and the pointers of entry point `name`: none null that may not be, each aligned
inline int check(int dtype, const char* name, std::initializer_list<Array> arrays) {
    PFB_REQUIRE(dtype == PFB_F32 || dtype == PFB_F64, PFB_ERR_INVALID, "%s: bad dtype %d", name, dtype);
    for (const Array& a : arrays) PFB_REQUIRE(a.ptr || a.optional, PFB_ERR_INVALID, "%s: null argument", name);
    for (const Array& a : arrays) {
        const size_t align = a.align.elems * esize(dtype) + a.align.bytes;
        PFB_REQUIRE(((uintptr_t)a.ptr & (align - 1)) == 0, PFB_ERR_INVALID, "%s: an array is not aligned to %zu bytes",
                    name, align);
    }
    return PFB_OK;
}
// nrow x nchan visibilities that an int indexes
inline int check_nvis(const char* name, size_t nrow, int nchan) {
    PFB_REQUIRE(nrow >= 1 && nchan >= 1 && nrow <= (size_t)0x7fffffff / (size_t)nchan, PFB_ERR_UNSUPPORTED,
                "%s: %zu rows x %d channels outside [1, 2^31)", name, nrow, nchan);
    return PFB_OK;
}
// as many elements; the file says whether anything else is invalid or unsupported
inline int check_count(const char* name, size_t n, int code) {
    PFB_REQUIRE(n >= 1 && n <= (size_t)0x7fffffff, code, "%s: %zu elements outside [1, 2^31)", name, n);
    return PFB_OK;
}

}  // namespace pfb
