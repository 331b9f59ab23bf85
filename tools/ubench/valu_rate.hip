// valu_rate.hip -- microbenchmark: how many lane-FMAs per second do v_fma_f32 / v_pk_fma_f32 sustain on
// gfx950 at 1, 2, 4 waves per SIMD?  Decides whether the sphere filter should be packed or not.
// Modes 5..: the operand forms of the sphere walk's node visit (rtx_traverse.h sphere_node_step_q3) at 4 waves per SIMD: what an SGPR,
// an SGPR-pair or a literal operand costs over the plain VGPR form of the same instruction.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
typedef float float2v __attribute__((ext_vector_type(2)));

template <int MODE>
__global__ void k(float *out, int iters, float a, float b)
{
    float x[16];
    float2v y[8];
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = threadIdx.x * 1e-3f + i;
#pragma unroll
    for (int i = 0; i < 8; ++i) y[i] = float2v{x[2 * i], x[2 * i + 1]};
    float2v a2 = {a, a}, b2 = {b, b};
    const uint32_t ua = __float_as_uint(a);
    const unsigned long long m64 = __ballot(threadIdx.x & 1);          // a lane mask in an SGPR pair
    double d[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = (double)x[i];
    const double da = (double)a;
    unsigned long long sink = 0;
    for (int it = 0; it < iters; ++it) {
        if (MODE == 0) {
#pragma unroll
            for (int i = 0; i < 16; ++i) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(x[i]) : "v"(a), "v"(b));
        } else if (MODE == 1) {
#pragma unroll
            for (int i = 0; i < 8; ++i) asm volatile("v_pk_fma_f32 %0, %0, %1, %2" : "+v"(y[i]) : "v"(a2), "v"(b2));
        } else if (MODE == 2) {  // fma with an SGPR operand
#pragma unroll
            for (int i = 0; i < 16; ++i) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(x[i]) : "s"(a), "v"(b));
        } else if (MODE == 3) {  // v_max3 + cmp mix
#pragma unroll
            for (int i = 0; i < 16; ++i) asm volatile("v_max3_f32 %0, %0, %1, %2" : "+v"(x[i]) : "v"(a), "v"(b));
        } else if (MODE == 4) {  // v_sub_f32
#pragma unroll
            for (int i = 0; i < 16; ++i) asm volatile("v_sub_f32 %0, %0, %1" : "+v"(x[i]) : "v"(a));
        } else if (MODE == 5) {  // literal operand
#pragma unroll
            for (int i = 0; i < 16; ++i) asm volatile("v_fmamk_f32 %0, %0, 0x3f800004, %1" : "+v"(x[i]) : "v"(b));
        } else if (MODE == 6) {  // VOP2 select on VCC (VCC written once per 16: nothing else in the block touches it)
            asm volatile("v_cmp_gt_f32_e32 vcc, %0, %1" : : "v"(a), "v"(x[0]) : "vcc");
#pragma unroll
            for (int i = 0; i < 16; ++i) asm volatile("v_cndmask_b32_e32 %0, %0, %1, vcc" : "+v"(x[i]) : "v"(a) : "vcc");
        } else if (MODE == 7) {  // VOP3 select on an SGPR pair
#pragma unroll
            for (int i = 0; i < 16; ++i) asm volatile("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(x[i]) : "v"(a), "s"(m64));
        } else if (MODE == 8) {  // compare into VCC
#pragma unroll
            for (int i = 0; i < 16; ++i) asm volatile("v_cmp_gt_f32_e32 vcc, %0, %1" : : "v"(a), "v"(x[i]) : "vcc");
        } else if (MODE == 9) {  // compare into an SGPR pair.  (Modes 9 and 10: the OR into `sink` puts an s_or_b64 that waits for the VALU-written
                                 // pair behind every compare -- these rows are an upper bound, mode 22 has the form without it)
#pragma unroll
            for (int i = 0; i < 16; ++i) { unsigned long long m; asm volatile("v_cmp_gt_f32_e64 %0, %1, %2" : "=s"(m) : "v"(a), "v"(x[i])); sink |= m; }
        } else if (MODE == 10) { // compare of an SGPR with a VGPR into an SGPR pair (the link-limit test)
#pragma unroll
            for (int i = 0; i < 16; ++i) { unsigned long long m; asm volatile("v_cmp_gt_u32_e64 %0, %1, %2" : "=s"(m) : "s"(ua), "v"(x[i])); sink |= m; }
        } else if (MODE == 11) { // compare of an SGPR with a VGPR into VCC (the +inf test)
#pragma unroll
            for (int i = 0; i < 16; ++i) asm volatile("v_cmp_lg_f32_e32 vcc, %0, %1" : : "s"(a), "v"(x[i]) : "vcc");
        } else if (MODE >= 12 && MODE <= 15) {  // byte -> f32
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if (MODE == 12) asm volatile("v_cvt_f32_ubyte0_e32 %0, %0" : "+v"(x[i]));
                if (MODE == 13) asm volatile("v_cvt_f32_ubyte1_e32 %0, %0" : "+v"(x[i]));
                if (MODE == 14) asm volatile("v_cvt_f32_ubyte2_e32 %0, %0" : "+v"(x[i]));
                if (MODE == 15) asm volatile("v_cvt_f32_ubyte3_e32 %0, %0" : "+v"(x[i]));
            }
        } else if (MODE == 16) { // the sort's compare-exchange: 8 min + 8 max
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                asm volatile("v_min_f64 %0, %0, %1" : "+v"(d[i]) : "v"(da));
                asm volatile("v_max_f64 %0, %0, %1" : "+v"(d[i]) : "v"(da));
            }
        } else if (MODE == 17) {
#pragma unroll
            for (int i = 0; i < 16; ++i) asm volatile("v_min3_f32 %0, %0, %1, %2" : "+v"(x[i]) : "v"(a), "v"(b));
        } else if (MODE == 18) { // two v_min for one v_min3: 32 instructions, counted as 16 (compare with twice the v_min row)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                asm volatile("v_min_f32_e32 %0, %0, %1" : "+v"(x[i]) : "v"(a));
                asm volatile("v_min_f32_e32 %0, %0, %1" : "+v"(x[i]) : "v"(b));
            }
        } else if (MODE == 19) {
#pragma unroll
            for (int i = 0; i < 16; ++i) asm volatile("v_min_f32_e32 %0, %0, %1" : "+v"(x[i]) : "v"(a));
        } else if (MODE == 20) { // v_bfi_b32 with VGPR sources: the select of the near / far words without an SGPR-pair mask
#pragma unroll
            for (int i = 0; i < 16; ++i) asm volatile("v_bfi_b32 %0, %1, %0, %2" : "+v"(x[i]) : "v"(a), "v"(b));
        } else if (MODE == 21) { // v_cmp (VCC) + VOP2 select, alternating: the per-child pair of the visit
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                asm volatile("v_cmp_gt_f32_e32 vcc, %0, %1" : : "v"(a), "v"(x[i]) : "vcc");
                asm volatile("v_cndmask_b32_e32 %0, %0, %1, vcc" : "+v"(x[i]) : "v"(a) : "vcc");
            }
        } else if (MODE == 22) { // v_cmp (SGPR pair) + VOP3 select, alternating
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                unsigned long long m;
                asm volatile("v_cmp_gt_f32_e64 %0, %1, %2" : "=s"(m) : "v"(a), "v"(x[i]));
                asm volatile("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(x[i]) : "v"(a), "s"(m));
            }
        }
    }
    float s = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += x[i];
#pragma unroll
    for (int i = 0; i < 8; ++i) s += y[i].x + y[i].y + (float)d[i];
    s += (float)(uint32_t)sink;
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

template <int MODE>
void run(const char *name, int waves_per_simd, int lanes_per_instr)
{
    int cus = 256;
    int threads = 256;                       // 4 waves per block = 1 per SIMD
    int blocks = cus * waves_per_simd;
    float *out;
    hipMalloc(&out, (size_t)blocks * threads * 4);
    int iters = 20000;
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    k<MODE><<<blocks, threads>>>(out, 100, 1.0001f, 0.5f);
    hipDeviceSynchronize();
    hipEventRecord(e0);
    k<MODE><<<blocks, threads>>>(out, iters, 1.0001f, 0.5f);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms;
    hipEventElapsedTime(&ms, e0, e1);
    double instr = (double)blocks * (threads / 64) * iters * (MODE == 1 ? 8 : 16);
    double laneops = instr * 64 * lanes_per_instr;
    // cycles per wave-instruction per SIMD assuming 2.4 GHz
    double simd_instr = instr / (cus * 4.0);
    printf("%-26s waves/SIMD %d: %.3f ms  %.2f T lane-ops/s  %.2f cyc/instr/SIMD @2.4GHz\n", name, waves_per_simd, ms,
           laneops / ms / 1e9, ms * 1e-3 * 2.4e9 / simd_instr);
    hipFree(out);
}

int main()
{
    for (int w : {1, 2, 4, 8}) {
        run<0>("v_fma_f32", w, 1);
        run<1>("v_pk_fma_f32", w, 2);
        run<2>("v_fma_f32 (sgpr src)", w, 1);
        run<3>("v_max3_f32", w, 1);
        run<4>("v_sub_f32", w, 1);
    }
    const int w = 4;                       // the node-visit forms: at the occupancy stage 2 runs at
    run<5>("v_fmamk_f32 (literal)", w, 1);
    run<19>("v_min_f32", w, 1);
    run<17>("v_min3_f32", w, 1);
    run<18>("2 x v_min_f32 (per pair)", w, 1);
    run<6>("v_cndmask e32 (vcc)", w, 1);
    run<7>("v_cndmask e64 (sgpr pair)", w, 1);
    run<20>("v_bfi_b32", w, 1);
    run<8>("v_cmp e32 -> vcc", w, 1);
    run<9>("v_cmp e64 -> sgpr pair", w, 1);
    run<10>("v_cmp_u32 e64 sgpr src", w, 1);
    run<11>("v_cmp e32 sgpr src", w, 1);
    run<21>("v_cmp+v_cndmask e32", w, 1);
    run<22>("v_cmp+v_cndmask e64", w, 1);
    run<12>("v_cvt_f32_ubyte0", w, 1);
    run<13>("v_cvt_f32_ubyte1", w, 1);
    run<14>("v_cvt_f32_ubyte2", w, 1);
    run<15>("v_cvt_f32_ubyte3", w, 1);
    run<16>("v_min_f64 / v_max_f64", w, 1);
    return 0;
}
