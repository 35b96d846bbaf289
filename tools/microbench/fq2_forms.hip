// The two forms of the Fq2 product (uzkge_amd/csrc/fq2_29.hpp) and the square as kernels of their own, for an instruction count:
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -I uzkge_amd/csrc -S --cuda-device-only tools/microbench/fq2_forms.hip -o fq2_forms.s
//   python tools/isa_hist.py fq2_forms.s fq2_mul_dual fq2_mul_kara fq2_sqr
// Operands and results are raw 29-bit limbs (normalized, values < 2 M as in the accumulator), so only the product is counted.
#include <hip/hip_runtime.h>

#include "fq2_29.hpp"

using namespace uzk;

struct Raw2 { L29 a, b; };

__device__ __forceinline__ q2::E2<1, 2> in2(const Raw2& r) { q2::E2<1, 2> x; x.a.v = r.a; x.b.v = r.b; return x; }
template <class T>
__device__ __forceinline__ Raw2 out2(const T& x) { Raw2 r; r.a = x.a.v; r.b = x.b.v; return r; }

extern "C" __global__ void fq2_mul_dual(const Raw2* a, const Raw2* b, Raw2* o) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    o[i] = out2(q2::mul(in2(a[i]), in2(b[i])));
}
extern "C" __global__ void fq2_mul_kara(const Raw2* a, const Raw2* b, Raw2* o) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    o[i] = out2(q2::mul_kara(in2(a[i]), in2(b[i])));
}
extern "C" __global__ void fq2_sqr(const Raw2* a, const Raw2* b, Raw2* o) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    o[i] = out2(q2::sqr(in2(a[i])));
}
