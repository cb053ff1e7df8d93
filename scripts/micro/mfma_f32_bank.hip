// Microbenchmark: does the VGPR bank of the A / B operands change the issue rate of v_mfma_f32_32x32x2_f32?
// 8 independent accumulators (a[0:127]) as in k_field_fwd_reg; A and B registers chosen by hand.
// hipcc --offload-arch=gfx950 -O3 mfma_f32_bank.hip -o mfma_f32_bank && ./mfma_f32_bank
#include <hip/hip_runtime.h>
#include <cstdio>

#define MF(acc, a, b) "v_mfma_f32_32x32x2_f32 a[" acc "], " a ", " b ", a[" acc "]\n\t"
#define EIGHT(a, b) MF("0:15", a, b) MF("16:31", a, b) MF("32:47", a, b) MF("48:63", a, b) MF("64:79", a, b) MF("80:95", a, b) MF("96:111", a, b) MF("112:127", a, b)
// four A registers per B as in the kernel (float4 fragment: consecutive registers = all four banks)
#define BLOCK_ROT(b) MF("0:15", "v4", b) MF("16:31", "v5", b) MF("32:47", "v6", b) MF("48:63", "v7", b) MF("64:79", "v8", b) MF("80:95", "v9", b) MF("96:111", "v10", b) MF("112:127", "v11", b)

// one MFMA followed by N independent VALU instructions
#define V1 "v_max_f32 v20, v21, v22\n\t"
#define MFV(acc, a, b, fill) MF(acc, a, b) fill
#define ROT_FILL(b, fill) MFV("0:15", "v4", b, fill) MFV("16:31", "v5", b, fill) MFV("32:47", "v6", b, fill) MFV("48:63", "v7", b, fill) MFV("64:79", "v8", b, fill) MFV("80:95", "v9", b, fill) MFV("96:111", "v10", b, fill) MFV("112:127", "v11", b, fill)
#define RD "ds_read_b128 v[24:27], v23\n\t"
#define ACR "v_accvgpr_read_b32 v20, a200\n\t"
// ---- what one lazy ReLU of 16 accumulator values (a[128:143]) costs per group of 32 MFMAs, by form (modes 10..16).
// v23 = lane * 16 and v22 = lane * 4 (LDS byte addresses; sh is the only LDS object, so it starts at 0), v21 = 0.
#define ROT_AT(b, f0, f1, f2, f3, f4, f5, f6, f7) MFV("0:15", "v4", b, f0) MFV("16:31", "v5", b, f1) MFV("32:47", "v6", b, f2) MFV("48:63", "v7", b, f3) MFV("64:79", "v8", b, f4) MFV("80:95", "v9", b, f5) MFV("96:111", "v10", b, f6) MFV("112:127", "v11", b, f7)
#define ROT_1(b, fill) ROT_AT(b, fill, "", "", "", "", "", "", "")
#define RM1(n, r) "v_accvgpr_read_b32 v20, a" #n "\n\tv_max_i32 " r ", 0, v20\n\t"
#define RM3(a, b, c) RM1(a, "v24") RM1(b, "v25") RM1(c, "v26")
#define RM2(a, b) RM1(a, "v27") RM1(b, "v28")
#define VMAX4(a, b, c, d) "v_max_i32 v" #a ", 0, v" #a "\n\tv_max_i32 v" #b ", 0, v" #b "\n\tv_max_i32 v" #c ", 0, v" #c "\n\tv_max_i32 v" #d ", 0, v" #d "\n\t"
#define VMAX16 VMAX4(24, 25, 26, 27) VMAX4(28, 29, 30, 31) VMAX4(32, 33, 34, 35) VMAX4(36, 37, 38, 39)
#define WR128 "ds_write_b128 v23, a[128:131]\n\tds_write_b128 v23, a[132:135] offset:1024\n\tds_write_b128 v23, a[136:139] offset:2048\n\tds_write_b128 v23, a[140:143] offset:3072\n\t"
#define RD128V "ds_read_b128 v[24:27], v23\n\tds_read_b128 v[28:31], v23 offset:1024\n\tds_read_b128 v[32:35], v23 offset:2048\n\tds_read_b128 v[36:39], v23 offset:3072\n\t"
#define RD128A "ds_read_b128 a[144:147], v23\n\tds_read_b128 a[148:151], v23 offset:1024\n\tds_read_b128 a[152:155], v23 offset:2048\n\tds_read_b128 a[156:159], v23 offset:3072\n\t"
#define W128(g) "ds_write_b128 v23, a[128+4*" #g ":131+4*" #g "] offset:1024*" #g "\n\t"
#define R128V(g) "ds_read_b128 v[24+4*" #g ":27+4*" #g "], v23 offset:1024*" #g "\n\t"
#define MX1(g, o) "ds_max_i32 v23, v21 offset:1024*" #g "+" #o "\n\t"
#define MXR(g, c) "ds_max_i32 v4" #c ", v21 offset:1024*" #g "\n\t"
#define MX4(o) "ds_max_i32 v23, v21 offset:" #o "\n\tds_max_i32 v23, v21 offset:" #o "+4\n\tds_max_i32 v23, v21 offset:" #o "+8\n\tds_max_i32 v23, v21 offset:" #o "+12\n\t"
#define MX128 MX4(0) MX4(1024) MX4(2048) MX4(3072)
// [register][lane] layout: register r of lane l at r * 256 + l * 4 (conflict-free for every b32 form)
#define W32(r) "ds_write_b32 v22, a" r " offset:(" r "-128)*256\n\t"
#define WR32 W32("128") W32("129") W32("130") W32("131") W32("132") W32("133") W32("134") W32("135") W32("136") W32("137") W32("138") W32("139") W32("140") W32("141") W32("142") W32("143")
#define M32(r) "ds_max_i32 v22, v21 offset:" #r "*256\n\t"
#define MX32 M32(0) M32(1) M32(2) M32(3) M32(4) M32(5) M32(6) M32(7) M32(8) M32(9) M32(10) M32(11) M32(12) M32(13) M32(14) M32(15)
#define R32(r) "ds_read_b32 v" r ", v22 offset:(" r "-24)*256\n\t"
#define RD32 R32("24") R32("25") R32("26") R32("27") R32("28") R32("29") R32("30") R32("31") R32("32") R32("33") R32("34") R32("35") R32("36") R32("37") R32("38") R32("39")
#define LGK0 "s_waitcnt lgkmcnt(0)\n\t"
#define RELU_REGS "memory", "v20", "v24", "v25", "v26", "v27", "v28", "v29", "v30", "v31", "v32", "v33", "v34", "v35", "v36", "v37", "v38", "v39", "a128", "a143", "a144", "a159"

template <int MODE>
__global__ __launch_bounds__(64) void k(unsigned long long* out, int iters) {
  __shared__ float sh[1024];
  sh[threadIdx.x] = 0.f;
  __syncthreads();
  unsigned long long t0 = 0, t1 = 0;
  asm volatile(
      "v_mov_b32 v4, 1.0\n\tv_mov_b32 v5, 1.0\n\tv_mov_b32 v6, 1.0\n\tv_mov_b32 v7, 1.0\n\t"
      "v_mov_b32 v8, 1.0\n\tv_mov_b32 v9, 1.0\n\tv_mov_b32 v10, 1.0\n\tv_mov_b32 v11, 1.0\n\tv_mov_b32 v12, 0.5\n\tv_mov_b32 v13, 0.5\n\t" ::
          : "v4", "v5", "v6", "v7", "v8", "v9", "v10", "v11", "v12", "v13");
  asm volatile("v_mbcnt_lo_u32_b32 v22, -1, 0\n\tv_mbcnt_hi_u32_b32 v22, -1, v22\n\tv_lshlrev_b32 v23, 4, v22\n\tv_lshlrev_b32 v22, 2, v22\n\tv_mov_b32 v21, 0\n\t"
               "v_mov_b32 v24, 0.5\n\tv_accvgpr_write_b32 a144, v24\n\t"
               // v40 + c = the lane's 16 bytes + 4 * ((c + lane / 8) & 3): the dword its c-th ds_max takes in the rotated form (mode 20)
               "v_lshrrev_b32 v44, 7, v23\n\t"
               "v_add_u32 v40, 0, v44\n\tv_add_u32 v41, 1, v44\n\tv_add_u32 v42, 2, v44\n\tv_add_u32 v43, 3, v44\n\t"
               "v_and_b32 v40, 3, v40\n\tv_and_b32 v41, 3, v41\n\tv_and_b32 v42, 3, v42\n\tv_and_b32 v43, 3, v43\n\t"
               "v_lshl_add_u32 v40, v40, 2, v23\n\tv_lshl_add_u32 v41, v41, 2, v23\n\tv_lshl_add_u32 v42, v42, 2, v23\n\tv_lshl_add_u32 v43, v43, 2, v23\n\t"
               ::: "v21", "v22", "v23", "v24", "a144", "v40", "v41", "v42", "v43", "v44");
  for (int i = 0; i < 128; ++i) asm volatile("" ::: "memory");
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0));
  for (int it = 0; it < iters; ++it) {
    if (MODE == 0) asm volatile(EIGHT("v4", "v8") EIGHT("v4", "v8") EIGHT("v4", "v8") EIGHT("v4", "v8")::: "memory");      // A, B same bank (4, 8)
    if (MODE == 1) asm volatile(EIGHT("v4", "v9") EIGHT("v4", "v9") EIGHT("v4", "v9") EIGHT("v4", "v9")::: "memory");      // different banks
    if (MODE == 2) asm volatile(BLOCK_ROT("v12") BLOCK_ROT("v12") BLOCK_ROT("v12") BLOCK_ROT("v12")::: "memory");        // kernel-like: A rotates over banks
    if (MODE == 3) asm volatile(EIGHT("v4", "v4") EIGHT("v4", "v4") EIGHT("v4", "v4") EIGHT("v4", "v4")::: "memory");      // same register
    if (MODE == 4) asm volatile(ROT_FILL("v12", V1 V1) ROT_FILL("v12", V1 V1) ROT_FILL("v12", V1 V1) ROT_FILL("v12", V1 V1)::: "memory", "v20");
    if (MODE == 5) asm volatile(ROT_FILL("v12", V1 V1 V1 V1 V1 V1 V1 V1) ROT_FILL("v12", V1 V1 V1 V1 V1 V1 V1 V1) ROT_FILL("v12", V1 V1 V1 V1 V1 V1 V1 V1) ROT_FILL("v12", V1 V1 V1 V1 V1 V1 V1 V1)::: "memory", "v20");
    if (MODE == 6) asm volatile(ROT_FILL("v12", V1 V1 V1 V1 V1 V1 V1 V1 V1 V1 V1 V1 V1 V1 V1 V1) ROT_FILL("v12", V1 V1 V1 V1 V1 V1 V1 V1 V1 V1 V1 V1 V1 V1 V1 V1) ROT_FILL("v12", V1 V1 V1 V1 V1 V1 V1 V1 V1 V1 V1 V1 V1 V1 V1 V1) ROT_FILL("v12", V1 V1 V1 V1 V1 V1 V1 V1 V1 V1 V1 V1 V1 V1 V1 V1)::: "memory", "v20");
    if (MODE == 7) asm volatile("v_mov_b32 v23, 0\n\t" ROT_FILL("v12", RD) ROT_FILL("v12", RD) ROT_FILL("v12", RD) ROT_FILL("v12", RD) "s_waitcnt lgkmcnt(0)\n\t" ::: "memory", "v23", "v24", "v25", "v26", "v27");
    if (MODE == 8) asm volatile(ROT_FILL("v12", ACR ACR) ROT_FILL("v12", ACR ACR) ROT_FILL("v12", ACR ACR) ROT_FILL("v12", ACR ACR)::: "memory", "v20");
    if (MODE == 9) asm volatile(ROT_FILL("v12", "s_waitcnt lgkmcnt(7)\n\t") ROT_FILL("v12", "s_waitcnt lgkmcnt(7)\n\t") ROT_FILL("v12", "s_waitcnt lgkmcnt(7)\n\t") ROT_FILL("v12", "s_waitcnt lgkmcnt(7)\n\t")::: "memory");
    // the request goes out behind the first MFMAs, the wait (and V1's v_max group) stands in front of MFMA 23, k-block 3 consumes:
    // 1,300 cycles of lead (the kernel has 4,096).  "burst": each kind of DS instruction behind one MFMA; "spread": one per MFMA
    if (MODE == 10) asm volatile(ROT_1("v12", RM3(128, 129, 130) RM3(131, 132, 133) RM3(134, 135, 136) RM3(137, 138, 139) RM2(140, 141) RM2(142, 143)) BLOCK_ROT("v12") BLOCK_ROT("v12") BLOCK_ROT("v24")::: RELU_REGS);
    if (MODE == 11) asm volatile(ROT_AT("v12", RM3(128, 129, 130), "", "", RM3(131, 132, 133), "", "", RM3(134, 135, 136), "") ROT_AT("v12", "", RM3(137, 138, 139), "", "", RM2(140, 141), "", "", RM2(142, 143)) BLOCK_ROT("v12") BLOCK_ROT("v24")::: RELU_REGS);
    if (MODE == 12) asm volatile(ROT_AT("v12", WR128, RD128V, "", "", "", "", "", "") BLOCK_ROT("v12") ROT_AT("v12", "", "", "", "", "", "", LGK0 VMAX16, "") BLOCK_ROT("v24")::: RELU_REGS);
    if (MODE == 13) asm volatile(ROT_AT("v12", W128(0), W128(1), W128(2), W128(3), R128V(0), R128V(1), R128V(2), R128V(3)) BLOCK_ROT("v12") ROT_AT("v12", "", "", "", "", "", "", LGK0 VMAX16, "") BLOCK_ROT("v24")::: RELU_REGS);
    if (MODE == 14) asm volatile(ROT_AT("v12", WR128, MX128, RD128V, "", "", "", "", "") BLOCK_ROT("v12") ROT_AT("v12", "", "", "", "", "", "", LGK0, "") BLOCK_ROT("v24")::: RELU_REGS);
    if (MODE == 15) asm volatile(ROT_AT("v12", W128(0), W128(1), W128(2), W128(3), MX1(0, 0), MX1(0, 4), MX1(0, 8), MX1(0, 12)) ROT_AT("v12", MX1(1, 0), MX1(1, 4), MX1(1, 8), MX1(1, 12), MX1(2, 0), MX1(2, 4), MX1(2, 8), MX1(2, 12))
                                 ROT_AT("v12", MX1(3, 0), MX1(3, 4), MX1(3, 8), MX1(3, 12), R128V(0), R128V(1), R128V(2), R128V(3)) ROT_AT("v12", "", "", "", "", "", "", LGK0, "")::: RELU_REGS);
    if (MODE == 16) asm volatile(ROT_AT("v12", WR128, MX128, RD128A, "", "", "", "", "") BLOCK_ROT("v12") ROT_AT("v12", "", "", "", "", "", "", LGK0, "") BLOCK_ROT("a144")::: RELU_REGS);
    if (MODE == 17) asm volatile(ROT_AT("v12", WR32, MX32, RD32, "", "", "", "", "") BLOCK_ROT("v12") ROT_AT("v12", "", "", "", "", "", "", LGK0, "") BLOCK_ROT("v24")::: RELU_REGS);
    if (MODE == 18) asm volatile(ROT_AT("v12", WR32, RD32, "", "", "", "", "", "") BLOCK_ROT("v12") ROT_AT("v12", "", "", "", "", "", "", LGK0 VMAX16, "") BLOCK_ROT("v24")::: RELU_REGS);
    if (MODE == 20) asm volatile(ROT_AT("v12", W128(0), MXR(0, 0), MXR(0, 1), MXR(0, 2), MXR(0, 3), R128V(0), W128(1), MXR(1, 0)) ROT_AT("v12", MXR(1, 1), MXR(1, 2), MXR(1, 3), R128V(1), W128(2), MXR(2, 0), MXR(2, 1), MXR(2, 2))
                                 ROT_AT("v12", MXR(2, 3), R128V(2), W128(3), MXR(3, 0), MXR(3, 1), MXR(3, 2), MXR(3, 3), R128V(3)) ROT_AT("v12", "", "", "", "", "", "", LGK0, "")::: RELU_REGS);
    if (MODE == 19) asm volatile(ROT_1("v12", VMAX16) BLOCK_ROT("v12") BLOCK_ROT("v12") BLOCK_ROT("v24")::: RELU_REGS);
  }
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1));
  if (threadIdx.x == 0) out[blockIdx.x] = t1 - t0;
}

template <int MODE>
void run(const char* label) {
  unsigned long long* out;
  hipMalloc(&out, 8 * 1024);
  const int iters = 2000;
  hipLaunchKernelGGL(k<MODE>, dim3(1024), dim3(64), 0, 0, out, 10);
  hipLaunchKernelGGL(k<MODE>, dim3(1024), dim3(64), 0, 0, out, iters);
  hipDeviceSynchronize();
  unsigned long long h[1024];
  hipMemcpy(h, out, sizeof(h), hipMemcpyDeviceToHost);
  double s = 0;
  for (int i = 0; i < 1024; ++i) s += (double)h[i];
  printf("%-42s %.2f ticks of s_memtime per MFMA (1 wave per SIMD, 1024 waves)\n", label, s / 1024 / iters / 32);
  hipFree(out);
}

int main() {
  run<0>("A, B in the same VGPR bank");
  run<1>("A, B in different banks");
  run<2>("A rotating over 8 registers, one B");
  run<3>("A = B (same register)");
  run<4>("+ 2 VALU (v_max_f32) per MFMA");
  run<5>("+ 8 VALU per MFMA");
  run<6>("+ 16 VALU per MFMA");
  run<7>("+ 1 ds_read_b128 per MFMA");
  run<8>("+ 2 v_accvgpr_read per MFMA");
  run<9>("+ 1 s_waitcnt lgkmcnt(7) per MFMA");
  // the lazy ReLU of one 16-register tile per 32 MFMAs (k_field_fwd_reg's activate()); 64.00 = free
  run<10>("V0  16 x (accvgpr_read + v_max_i32), 1 group");
  run<11>("V0  the same in six groups");
  run<19>("    16 v_max_i32 alone, 1 group");
  run<12>("V1  4 ds_write_b128 (AGPR), 4 ds_read_b128, 16 v_max: burst");
  run<13>("V1  the same, one DS per MFMA");
  run<14>("V2  b128 write, 16 ds_max_i32, read to VGPR: burst");
  run<15>("V2  the same, one DS per MFMA");
  run<20>("V2  one DS per MFMA, group by group, ds_max dwords rotated");
  run<16>("V2  burst, read to AGPR, B operand = AGPR");
  run<17>("V3  [reg][lane] b32: write, ds_max_i32, read: burst");
  run<18>("V3' [reg][lane] b32: write, read, 16 v_max: burst");
  return 0;
}
