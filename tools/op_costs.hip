// Micro-benchmark: issue cost of every vector instruction the class walk of score_kernel is made of, one stream per opcode,
// at 6 and at 8 waves per SIMD (the class variants run at 6).  A sibling of tools/valu_peak.hip, which measured mixes the
// compiler chose; here every instruction is pinned with a one-instruction asm, so the opcode and its operand kinds
// (VOP2 / VOP3, a scalar source or not) are what the stream's name says.
//   hipcc -O3 --offload-arch=gfx950 -o op_costs tools/op_costs.hip && ./op_costs
//   hipcc -O3 --offload-arch=gfx950 -S --cuda-device-only -o op_costs.s tools/op_costs.hip     (the opcodes, to check)
// Every wave runs 16 independent chains; a chain's instruction reads its own last result and one or two other
// registers.  The waves per SIMD are set by the LDS a workgroup asks for (160 KB per CU: 26 KB lets six workgroups of
// four waves in, 20 KB eight), the grid is four rounds of that.  Output: one line per (stream, waves), cycles per wave64
// instruction at the clock the device reports.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

enum Op { MOV, AND, OR, XOR, BFI_S, BITOP3_ANDN, BITOP3_ORAND, ALIGNBIT_S, BCNT, ALIGN_AND, ALIGN_ANDN, N_OPS };

// one instruction (two for the mixes) on chain a, other operands b, c (vector) and s (scalar)
template <int OP>
__device__ __forceinline__ void step(uint32_t &a, uint32_t b, uint32_t c, uint32_t s) {
    uint32_t t;
    if constexpr (OP == MOV) asm volatile("v_mov_b32_e32 %0, %1" : "=v"(a) : "v"(b));
    if constexpr (OP == AND) asm volatile("v_and_b32_e32 %0, %1, %0" : "+v"(a) : "v"(b));
    if constexpr (OP == OR) asm volatile("v_or_b32_e32 %0, %1, %0" : "+v"(a) : "v"(b));
    if constexpr (OP == XOR) asm volatile("v_xor_b32_e32 %0, %1, %0" : "+v"(a) : "v"(b));
    if constexpr (OP == BFI_S) asm volatile("v_bfi_b32 %0, %3, %1, %2" : "=v"(a) : "v"(b), "v"(a), "s"(s));          // (s & b) | (~s & a)
    if constexpr (OP == BITOP3_ANDN) asm volatile("v_bitop3_b32 %0, %0, %1, %0 bitop3:0x30" : "+v"(a) : "v"(b));      // a & ~b
    if constexpr (OP == BITOP3_ORAND) asm volatile("v_bitop3_b32 %0, %0, %1, %2 bitop3:0xc8" : "+v"(a) : "v"(b), "v"(c));   // (a | b) & c
    if constexpr (OP == ALIGNBIT_S) asm volatile("v_alignbit_b32 %0, %0, %1, %2" : "+v"(a) : "v"(b), "s"(s));
    if constexpr (OP == BCNT) asm volatile("v_bcnt_u32_b32 %0, %1, %0" : "+v"(a) : "v"(b));
    if constexpr (OP == ALIGN_AND) {        // a positive constraint of the walk
        asm volatile("v_alignbit_b32 %0, %1, %2, %3" : "=v"(t) : "v"(b), "v"(c), "s"(s));
        asm volatile("v_and_b32_e32 %0, %1, %0" : "+v"(a) : "v"(t));
    }
    if constexpr (OP == ALIGN_ANDN) {       // a negative one
        asm volatile("v_alignbit_b32 %0, %1, %2, %3" : "=v"(t) : "v"(b), "v"(c), "s"(s));
        asm volatile("v_bitop3_b32 %0, %0, %1, %0 bitop3:0x30" : "+v"(a) : "v"(t));
    }
}

template <int OP>
__global__ __launch_bounds__(256) void stream(uint32_t *out, uint32_t seed, int iters) {
    extern __shared__ uint32_t occupancy_pad[];
    uint32_t a[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = seed * (threadIdx.x + 1) + i * 0x9E3779B9u;
    const uint32_t s = __builtin_amdgcn_readfirstlane(seed & 31u) | 1u;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int i = 0; i < 16; ++i) step<OP>(a[i], a[(i + 1) & 15], a[(i + 5) & 15], s);
        }
    }
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) r ^= a[i];
    if (seed == 0xFFFFFFFFu) occupancy_pad[threadIdx.x] = r;    // (never: keeps the allocation)
    out[(size_t)blockIdx.x * 256 + threadIdx.x] = r;
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

template <int OP>
static void run(const char *name, int instr_per_step, int waves_per_simd, int cus, double hz) {
    const int per_cu = waves_per_simd;                      // workgroups of four waves per CU
    const size_t lds = waves_per_simd == 6 ? 26 * 1024 : 20 * 1024;
    const int blocks = cus * per_cu * 4, iters = 1024;
    uint32_t *d;
    CHECK(hipMalloc(&d, (size_t)blocks * 256 * sizeof(uint32_t)));
    int resident = 0;
    CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, stream<OP>, 256, lds));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    hipLaunchKernelGGL(stream<OP>, dim3(blocks), dim3(256), lds, 0, d, 12345u, 16);
    CHECK(hipDeviceSynchronize());
    double best = 1e30;
    for (int rep = 0; rep < 3; ++rep) {
        CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL(stream<OP>, dim3(blocks), dim3(256), lds, 0, d, 12345u, iters);
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        float ms;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (ms < best) best = ms;
    }
    const double winstr = (double)blocks * 4 * iters * 64 * instr_per_step;      // wave-instructions of the launch
    const double per_simd_s = winstr / (best * 1e-3) / (cus * 4.0);
    printf("%-22s waves/SIMD %d (resident workgroups/CU %d)  %8.3f ms  %.3f cycles per wave64 instruction\n", name, waves_per_simd,
           resident, best, hz / per_simd_s);
    CHECK(hipEventDestroy(e0));
    CHECK(hipEventDestroy(e1));
    CHECK(hipFree(d));
}

int main() {
    int cus = 0, khz = 0;
    CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
    CHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeClockRate, 0));
    printf("device: %d CUs, reported clock %.3f GHz; 16 chains per wave, 4 waves per workgroup\n", cus, khz * 1e-6);
    const double hz = khz * 1e3;
    for (int w : {6, 8}) {
        run<MOV>("v_mov_b32", 1, w, cus, hz);
        run<AND>("v_and_b32 (VOP2)", 1, w, cus, hz);
        run<OR>("v_or_b32 (VOP2)", 1, w, cus, hz);
        run<XOR>("v_xor_b32 (VOP2)", 1, w, cus, hz);
        run<BFI_S>("v_bfi_b32 s,v,v", 1, w, cus, hz);
        run<BITOP3_ANDN>("v_bitop3 0x30 a&~b", 1, w, cus, hz);
        run<BITOP3_ORAND>("v_bitop3 0xc8 (a|b)&c", 1, w, cus, hz);
        run<ALIGNBIT_S>("v_alignbit_b32 v,v,s", 1, w, cus, hz);
        run<BCNT>("v_bcnt_u32_b32", 1, w, cus, hz);
        run<ALIGN_AND>("alignbit + and", 2, w, cus, hz);
        run<ALIGN_ANDN>("alignbit + bitop3 0x30", 2, w, cus, hz);
    }
    return 0;
}
