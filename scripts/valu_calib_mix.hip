// valu_calib_mix.hip — issue cost on gfx950 of the instructions the mixed-precision inner step is made of (rt_device.h: trav_inner<.., .., true>):
// v_perm_b32, v_fma_mix_f32 with a normal and with a DENORMAL fp16 multiplicand (low and high half), v_ldexp_f32 — each alone and alternating
// 1 : 1 with v_fma_f32 — and the two decodes of a pair of planes side by side: cvt, fma, cvt, fma against perm, mix, mix.
// Method of profiles/r03_valu_calibration2.json: 6 waves per SIMD (one workgroup of 4 waves per 1/6 of a CU's LDS, 6 x CUs workgroups), every
// wave issues ITER x 128 instructions of the stream from one inline-asm block on 8 independent accumulators, and times itself on the shader's
// cycle counter and on the chip-wide 100 MHz clock. cycles per instruction and SIMD = wave cycles / (6 x instructions). The MODE register is
// not touched: fp16 denormals are on, as in every kernel hipcc compiles.
// It also checks the arithmetic the step relies on: for all 256 bytes in either half, perm + v_fma_mix_f32 on a * 2^24 against fmaf((float)q, a, b).
//   hipcc --offload-arch=gfx950 -O2 scripts/valu_calib_mix.hip -o valu_calib_mix && ./valu_calib_mix out.json
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define CHECK(x)                                                                          \
    do {                                                                                  \
        hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess) {                                                           \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                       \
            return 2;                                                                     \
        }                                                                                 \
    } while (0)

constexpr int kIter = 4096, kBlockInstr = 128, kWavesPerSimd = 6;
constexpr uint32_t kPermLo = 0x0C010C00u, kPermHi = 0x0C030C02u;

// one instruction of the stream per line; %0 .. %7 accumulators, %8 x, %9 y, %10 plane word, %11 normal halves, %12 denormal halves, %13 selector
#define FMA(A) "v_fma_f32 " A ", %8, %9, " A "\n"
#define CVT(A) "v_cvt_f32_ubyte0 " A ", %10\n"
#define CVT1(A) "v_cvt_f32_ubyte1 " A ", %10\n"
#define PERM(A) "v_perm_b32 " A ", %10, %10, %13\n"
#define MIXN(A) "v_fma_mix_f32 " A ", %11, %9, " A " op_sel_hi:[1,0,0]\n"
#define MIXD(A) "v_fma_mix_f32 " A ", %12, %9, " A " op_sel_hi:[1,0,0]\n"
#define MIXDH(A) "v_fma_mix_f32 " A ", %12, %9, " A " op_sel:[1,0,0] op_sel_hi:[1,0,0]\n"
#define LDEXP(A) "v_ldexp_f32 " A ", %8, 24\n"
#define ANDL(A) "v_and_b32 " A ", 0xff00ff, %10\n"        /* {0, b2, 0, b0}: the even bytes as halves, no selector register */
#define PKSHR(A) "v_pk_lshrrev_b16 " A ", 8, %10\n"      /* {0, b3, 0, b1}: the odd bytes */
#define ALONE(OP) OP("%0") OP("%1") OP("%2") OP("%3") OP("%4") OP("%5") OP("%6") OP("%7")
#define ALT(OP) FMA("%0") OP("%4") FMA("%1") OP("%5") FMA("%2") OP("%6") FMA("%3") OP("%7")
// a pair of planes as the parent decodes it (4 instructions) and as the mixed step does (3): 24 of each make a block of 96 / 72
#define PAIR_CVT CVT("%4") FMA("%0") CVT1("%5") FMA("%1") CVT("%6") FMA("%2") CVT1("%7") FMA("%3")
#define PAIR_MIX PERM("%4") MIXD("%0") MIXDH("%1") PERM("%5") MIXD("%2") MIXDH("%3")
#define PAIR_MIX2 ANDL("%4") MIXD("%0") MIXDH("%1") PKSHR("%5") MIXD("%2") MIXDH("%3")

struct Stream {
    const char* op;
    int block; // instructions per asm block
    int planes; // plane values per block (0: not a decode)
};
static const Stream kStreams[] = {
    {"v_fma_f32", 128, 0},
    {"v_cvt_f32_ubyte0", 128, 0},
    {"v_perm_b32 (selector in an SGPR)", 128, 0},
    {"v_fma_mix_f32, fp16 multiplicand NORMAL (0x3cab), low half", 128, 0},
    {"v_fma_mix_f32, fp16 multiplicand DENORMAL (0x00ab), low half", 128, 0},
    {"v_fma_mix_f32, fp16 multiplicand DENORMAL (0x00ab), high half (op_sel)", 128, 0},
    {"v_ldexp_f32 (inline 24)", 128, 0},
    {"alternating v_fma_f32 / v_cvt_f32_ubyte0", 128, 0},
    {"alternating v_fma_f32 / v_perm_b32", 128, 0},
    {"alternating v_fma_f32 / v_fma_mix_f32 normal", 128, 0},
    {"alternating v_fma_f32 / v_fma_mix_f32 denormal", 128, 0},
    {"alternating v_fma_f32 / v_ldexp_f32", 128, 0},
    {"plane decode today: cvt, fma, cvt, fma (4 instructions per 2 planes)", 128, 64},
    {"plane decode mixed: perm, mix lo, mix hi (3 instructions per 2 planes, denormal halves)", 96, 64},
    {"alternating v_perm_b32 / v_fma_mix_f32 denormal", 128, 0},
    {"v_and_b32 with a 32-bit literal", 128, 0},
    {"v_pk_lshrrev_b16 (inline 8)", 128, 0},
    {"plane decode mixed, no selector: and / pk_lshr, mix lo, mix hi (3 instructions per 2 planes)", 96, 64},
    {"alternating v_fma_f32 / v_pk_lshrrev_b16", 128, 0},
};
constexpr int kNumStreams = (int)(sizeof(kStreams) / sizeof(kStreams[0]));

template <int S>
__global__ void __launch_bounds__(256) k_stream(unsigned long long* __restrict__ out, float* __restrict__ sink) {
    __shared__ char occupancy_pad[26 * 1024]; // six workgroups fill a CU's 160 KiB: 6 waves per SIMD, no more
    occupancy_pad[threadIdx.x] = (char)threadIdx.x;
    __syncthreads();
    float a0 = occupancy_pad[(threadIdx.x + 1) & 255] * 1e-9f, a1 = 1.0f, a2 = 2.0f, a3 = 3.0f, a4 = 4.0f, a5 = 5.0f, a6 = 6.0f, a7 = 7.0f;
    const float x = 1.0f, y = 1.0e-3f;
    const uint32_t w = 0x11ab22cdu + threadIdx.x, hn = 0x3cab3cabu, hd = 0x00ab00abu, selector = kPermLo;
    const unsigned long long r0 = wall_clock64();
    const long long t0 = (long long)__builtin_readcyclecounter();
    for (int i = 0; i < kIter; ++i) {
#define BLOCK(TEXT) asm volatile(TEXT : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(x), "v"(y), "v"(w), "v"(hn), "v"(hd), "s"(selector))
        if (S == 0) BLOCK(".rept 16\n" ALONE(FMA) ".endr");
        if (S == 1) BLOCK(".rept 16\n" ALONE(CVT) ".endr");
        if (S == 2) BLOCK(".rept 16\n" ALONE(PERM) ".endr");
        if (S == 3) BLOCK(".rept 16\n" ALONE(MIXN) ".endr");
        if (S == 4) BLOCK(".rept 16\n" ALONE(MIXD) ".endr");
        if (S == 5) BLOCK(".rept 16\n" ALONE(MIXDH) ".endr");
        if (S == 6) BLOCK(".rept 16\n" ALONE(LDEXP) ".endr");
        if (S == 7) BLOCK(".rept 16\n" ALT(CVT) ".endr");
        if (S == 8) BLOCK(".rept 16\n" ALT(PERM) ".endr");
        if (S == 9) BLOCK(".rept 16\n" ALT(MIXN) ".endr");
        if (S == 10) BLOCK(".rept 16\n" ALT(MIXD) ".endr");
        if (S == 11) BLOCK(".rept 16\n" ALT(LDEXP) ".endr");
        if (S == 12) BLOCK(".rept 16\n" PAIR_CVT ".endr");
        if (S == 13) BLOCK(".rept 16\n" PAIR_MIX ".endr");
        if (S == 14) BLOCK(".rept 16\n" PERM("%4") MIXD("%0") PERM("%5") MIXD("%1") PERM("%6") MIXD("%2") PERM("%7") MIXD("%3") ".endr");
        if (S == 15) BLOCK(".rept 16\n" ALONE(ANDL) ".endr");
        if (S == 16) BLOCK(".rept 16\n" ALONE(PKSHR) ".endr");
        if (S == 17) BLOCK(".rept 16\n" PAIR_MIX2 ".endr");
        if (S == 18) BLOCK(".rept 16\n" ALT(PKSHR) ".endr");
#undef BLOCK
    }
    const long long t1 = (long long)__builtin_readcyclecounter();
    const unsigned long long r1 = wall_clock64();
    if ((threadIdx.x & 63u) == 0u) {
        const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6);
        out[2 * wave] = (unsigned long long)(t1 - t0), out[2 * wave + 1] = r1 - r0;
    }
    if (a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7 == 12345.678f) sink[0] = a0; // keeps the accumulators alive
}

// the arithmetic: lane q of 256 holds byte q in both halves' low bytes; out = {mixed low, mixed high, fmaf} bits for each (a, b)
__global__ void __launch_bounds__(256) k_check(const float* __restrict__ ab, int n, uint32_t* __restrict__ out) {
    const uint32_t q = threadIdx.x;
    const uint32_t word = q | ((255u - q) << 8) | (q << 16) | ((q ^ 0x5au) << 24);
    uint32_t lo, hi;
    const uint32_t sel_lo = kPermLo, sel_hi = kPermHi;
    asm volatile("v_perm_b32 %0, %1, %1, %2" : "=v"(lo) : "v"(word), "s"(sel_lo));
    asm volatile("v_perm_b32 %0, %1, %1, %2" : "=v"(hi) : "v"(word), "s"(sel_hi));
    for (int i = 0; i < n; ++i) {
        const float a = ab[2 * i], b = ab[2 * i + 1];
        const float am = __builtin_ldexpf(a, 24);
        float m0, m1;
        asm volatile("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(m0) : "v"(lo), "v"(am), "v"(b));
        asm volatile("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(m1) : "v"(hi), "v"(am), "v"(b));
        uint32_t* o = out + ((size_t)i * 256u + q) * 6u;
        o[0] = __float_as_uint(m0), o[1] = __float_as_uint(__builtin_fmaf((float)q, a, b));               // byte 0 through the low half of `lo`
        o[2] = __float_as_uint(m1), o[3] = __float_as_uint(__builtin_fmaf((float)(q ^ 0x5au), a, b));     // byte 3 through the high half of `hi`
        o[4] = lo, o[5] = hi;
    }
}

template <int S>
static int run_stream(int blocks, unsigned long long* d_out, float* d_sink, std::vector<unsigned long long>& h, double& cyc, double& ref) {
    k_stream<S><<<blocks, 256>>>(d_out, d_sink); // warm-up: code object load, clocks
    k_stream<S><<<blocks, 256>>>(d_out, d_sink);
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(h.data(), d_out, h.size() * sizeof(h[0]), hipMemcpyDeviceToHost));
    double c = 0, r = 0;
    for (size_t i = 0; i < h.size() / 2; ++i) c += (double)h[2 * i], r += (double)h[2 * i + 1];
    cyc = c / (double)(h.size() / 2), ref = r / (double)(h.size() / 2);
    return 0;
}

template <int S>
static int run_all(int blocks, unsigned long long* d_out, float* d_sink, std::vector<unsigned long long>& h, double* cyc, double* ref) {
    if (int e = run_stream<S>(blocks, d_out, d_sink, h, cyc[S], ref[S])) return e;
    if constexpr (S + 1 < kNumStreams) return run_all<S + 1>(blocks, d_out, d_sink, h, cyc, ref);
    return 0;
}

int main(int argc, char** argv) {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount, blocks = cus * kWavesPerSimd;
    unsigned long long* d_out;
    float* d_sink;
    CHECK(hipMalloc(&d_out, (size_t)blocks * 4 * 2 * sizeof(unsigned long long)));
    CHECK(hipMalloc(&d_sink, 64));
    std::vector<unsigned long long> h((size_t)blocks * 4 * 2);

    // the arithmetic first
    std::vector<float> ab;
    const float as[] = {1.0f, -1.0f, 0.37f, 3.1e-7f, -7.7e12f, 0x1p-20f * 0x1p83f, -0x1p20f * 0x1p83f, 1.17549435e-38f, 1e-41f, 5.5e24f, 0.0f};
    const float bs[] = {0.0f, -0.0f, 1.0f, -255.37f, 9.1e15f, -3.3e27f, 1e-40f, 2.9e34f, -1e8f * 0x1p83f};
    for (float a : as)
        for (float b : bs) ab.push_back(a), ab.push_back(b);
    const int n = (int)ab.size() / 2;
    float* d_ab;
    uint32_t* d_chk;
    CHECK(hipMalloc(&d_ab, ab.size() * sizeof(float)));
    CHECK(hipMalloc(&d_chk, (size_t)n * 256 * 6 * sizeof(uint32_t)));
    CHECK(hipMemcpy(d_ab, ab.data(), ab.size() * sizeof(float), hipMemcpyHostToDevice));
    k_check<<<1, 256>>>(d_ab, n, d_chk);
    CHECK(hipDeviceSynchronize());
    std::vector<uint32_t> chk((size_t)n * 256 * 6);
    CHECK(hipMemcpy(chk.data(), d_chk, chk.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    long bad = 0, bad_perm = 0, total = 0;
    for (int i = 0; i < n; ++i)
        for (uint32_t q = 0; q < 256; ++q) {
            const uint32_t* o = &chk[((size_t)i * 256 + q) * 6];
            total += 2;
            for (int k = 0; k < 2; ++k)
                if (o[2 * k] != o[2 * k + 1] && !(std::isnan(*(const float*)&o[2 * k]) && std::isnan(*(const float*)&o[2 * k + 1]))) {
                    if (bad++ < 8) fprintf(stderr, "mismatch: q %u half %d a %g b %g: mixed %08x fmaf %08x\n", q, k, ab[2 * i], ab[2 * i + 1], o[2 * k], o[2 * k + 1]);
                }
            if (o[4] != (q | ((255u - q) << 16)) || o[5] != (q | ((q ^ 0x5au) << 16))) bad_perm++;
        }
    printf("arithmetic: %ld results, %ld differ from fmaf((float)q, a, b); %ld perm words wrong\n", total, bad, bad_perm);

    double cyc[kNumStreams], ref[kNumStreams];
    if (int e = run_all<0>(blocks, d_out, d_sink, h, cyc, ref)) return e;
    FILE* f = argc > 1 ? fopen(argv[1], "w") : stdout;
    if (!f) return 3;
    fprintf(f, "{\n \"source\": \"scripts/valu_calib_mix.hip on %s: %d CUs, %d waves per SIMD, %d x %d instructions per wave; wave cycles on the shader cycle counter / (waves per SIMD x instructions); MODE register untouched (fp16 denormals on)\",\n",
            prop.gcnArchName, cus, kWavesPerSimd, kIter, kBlockInstr);
    fprintf(f, " \"arithmetic\": {\"results\": %ld, \"differ_from_fmaf\": %ld, \"perm_words_wrong\": %ld},\n \"streams\": [\n", total, bad, bad_perm);
    for (int s = 0; s < kNumStreams; ++s) {
        const double instr = (double)kIter * kStreams[s].block;
        const double cpi = cyc[s] / (kWavesPerSimd * instr);
        const double ref_cpi = ref[s] / (kWavesPerSimd * instr);
        fprintf(f, "  {\"op\": \"%s\", \"cycles_per_instruction_per_simd_6_waves\": %.3f, \"relative_to_v_fma_f32\": %.3f, \"ticks_100MHz_per_instruction\": %.5f", kStreams[s].op, cpi,
                cyc[s] / instr / (cyc[0] / ((double)kIter * kStreams[0].block)), ref_cpi);
        if (kStreams[s].planes) fprintf(f, ", \"cycles_per_plane\": %.3f", cyc[s] / (kWavesPerSimd * (double)kIter * kStreams[s].planes));
        fprintf(f, "}%s\n", s + 1 < kNumStreams ? "," : "");
        printf("%-90s %.3f cycles / instruction\n", kStreams[s].op, cpi);
    }
    fprintf(f, " ]\n}\n");
    if (f != stdout) fclose(f);
    return bad || bad_perm ? 1 : 0;
}
