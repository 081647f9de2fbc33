// What the scalar side of a wave's instruction stream costs on gfx950 (DESIGN
// §2.1t): cycles per instruction of
//   fma     v_fma_f32 alone (the yardstick);
//   mask    s_and_b64 of an SGPR pair with exec;
//   cmpand  v_cmp_lt_f32 into vcc + s_and_b64 of vcc into an SGPR pair (per pair);
//   execz   s_cbranch_execz, not taken (exec is never empty);
//   branch  s_branch, taken, to the next instruction;
//   loop    a counted back-edge: s_sub_u32, s_cmp_lg_u32, s_cbranch_scc1 taken (per iteration);
// each alone and interleaved one to one with independent v_fma_f32, at one wave
// per SIMD (one block of 256 threads) and at five (blocks of 256 threads with
// 30 KB of LDS each: five fit a CU's 160 KB and a sixth does not; five per CU launched).  Fixed trip
// counts, one short launch per case: kIter iterations of kRep copies.  Each
// wave brackets its loop with s_memtime (shader cycles); the table holds the
// median over waves, and for the interleaved rows the cycles per (scalar + fma)
// pair, so "pair - fma alone" is what the scalar instruction adds beside VALU.
// build: hipcc -O2 --offload-arch=gfx950 tools/issue_probe.hip -o issue_probe
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); std::exit(1); } } while (0)

constexpr int kIter = 256, kRep = 64;   // (the counting loop around a block of 64 adds under 5 %)

#define R2(x) x x
#define R4(x) R2(x) R2(x)
#define R16(x) R4(x) R4(x) R4(x) R4(x)
#define R64(x) R16(x) R16(x) R16(x) R16(x)

#define FMA "v_fma_f32 %[a], %[a], %[c], %[c]\n\t"
#define MASK "s_and_b64 %[m], %[m], exec\n\t"
#define CMPAND "v_cmp_lt_f32_e32 vcc, %[c], %[b]\n\ts_and_b64 %[m], vcc, %[m]\n\t"
#define EXECZ "s_cbranch_execz 9f\n\t"
#define BRANCH "s_branch 1f\n1:\n\t"

enum Case { kFma, kMask, kCmpAnd, kExecz, kBranch, kLoop, kCases };
static const char* kNames[kCases] = {"fma", "mask", "cmpand", "execz", "branch", "loop"};

// one case: kIter iterations of kRep copies of S, with an fma after each when WITH_FMA
template <int CASE, bool WITH_FMA>
__global__ void probe(unsigned long long* out, float seed) {
  extern __shared__ float lds[];   // (sized by the launch to set the blocks per CU; not read)
  float a = seed + threadIdx.x, b = seed * 0.5f, c = 1.0f + seed;
  unsigned long long m = ~0ull;
  unsigned int n = 0;
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll 1
  for (int i = 0; i < kIter; ++i) {
#define BODY(S) asm volatile(R64(S) "9:" : [a] "+v"(a), [m] "+s"(m), [n] "+s"(n) : [b] "v"(b), [c] "v"(c) : "vcc", "scc")
    if (CASE == kFma) BODY(FMA);
    else if (CASE == kMask && !WITH_FMA) BODY(MASK);
    else if (CASE == kMask) BODY(MASK FMA);
    else if (CASE == kCmpAnd && !WITH_FMA) BODY(CMPAND);
    else if (CASE == kCmpAnd) BODY(CMPAND FMA);
    else if (CASE == kExecz && !WITH_FMA) BODY(EXECZ);
    else if (CASE == kExecz) BODY(EXECZ FMA);
    else if (CASE == kBranch && !WITH_FMA) BODY(BRANCH);
    else if (CASE == kBranch) BODY(BRANCH FMA);
    else if (CASE == kLoop && !WITH_FMA)
      asm volatile("s_mov_b32 %[n], 64\n1:\n\ts_sub_u32 %[n], %[n], 1\n\ts_cmp_lg_u32 %[n], 0\n\ts_cbranch_scc1 1b"
                   : [n] "+s"(n) : : "scc");
    else
      asm volatile("s_mov_b32 %[n], 64\n1:\n\t" FMA "s_sub_u32 %[n], %[n], 1\n\ts_cmp_lg_u32 %[n], 0\n\ts_cbranch_scc1 1b"
                   : [a] "+v"(a), [n] "+s"(n) : [c] "v"(c) : "scc");
#undef BODY
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  const unsigned int wave = (blockIdx.x * blockDim.x + threadIdx.x) / 64u;
  // (a and m are kept live; one lane of each wave writes its cycles, the last lane the sink)
  if ((threadIdx.x & 63u) == 0u) out[wave] = t1 - t0;
  if (a == 12345.678f && m == 3ull) out[wave] = 0ull;
}

template <int CASE, bool WITH_FMA>
double run(int blocks, size_t lds, unsigned long long* dev, std::vector<unsigned long long>& host) {
  const int waves = blocks * 4;
  CHECK(hipMemset(dev, 0, host.size() * sizeof(unsigned long long)));
  hipLaunchKernelGGL((probe<CASE, WITH_FMA>), dim3(blocks), dim3(256), lds, 0, dev, 0.25f);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(host.data(), dev, waves * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  std::vector<unsigned long long> v(host.begin(), host.begin() + waves);
  std::nth_element(v.begin(), v.begin() + waves / 2, v.end());
  return (double)v[waves / 2] / ((double)kIter * kRep);
}

template <int CASE>
void rows(int cus, unsigned long long* dev, std::vector<unsigned long long>& host) {
  const size_t lds5 = 30 * 1024;
  const double a1 = run<CASE, false>(1, 0, dev, host), f1 = run<CASE, true>(1, 0, dev, host);
  const double a5 = run<CASE, false>(cus * 5, lds5, dev, host), f5 = run<CASE, true>(cus * 5, lds5, dev, host);
  std::printf("| %s | %.2f | %.2f | %.2f | %.2f |\n", kNames[CASE], a1, f1, a5, f5);
}

int main() {
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount;
  std::vector<unsigned long long> host((size_t)cus * 5 * 4);
  unsigned long long* dev;
  CHECK(hipMalloc(&dev, host.size() * sizeof(unsigned long long)));
  std::printf("%s, %d CUs; shader cycles per instruction (cmpand: per pair, loop: per iteration), median over waves\n",
              prop.gcnArchName, cus);
  std::printf("| case | alone, 1 wave/SIMD | + v_fma each, 1 wave/SIMD | alone, 5 waves/SIMD | + v_fma each, 5 waves/SIMD |\n");
  std::printf("|---|---|---|---|---|\n");
  rows<kFma>(cus, dev, host);
  rows<kMask>(cus, dev, host);
  rows<kCmpAnd>(cus, dev, host);
  rows<kExecz>(cus, dev, host);
  rows<kBranch>(cus, dev, host);
  rows<kLoop>(cus, dev, host);
  CHECK(hipFree(dev));
  return 0;
}
