// One-wave probe of v_mfma_scale_f32_16x16x128_f8f6f4 with an fp8 A and an fp4 B operand: which k
// each lane's elements are, which lane's scale byte applies to which block, which byte op_sel reads
// (docs/kernels.md "MXFP4 evaluation"; the recorded output is profiles/mxfp4/instruction_probe.txt).
// hipcc --offload-arch=gfx950 -O2 -o mx4_probe mx4_probe.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

template <int OSA, int OSB>
__global__ void probe(const int* a, const int* b, const int* sa, const int* sb, float* out) {
  const int l = threadIdx.x;
  i32x8 av, bv = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int j = 0; j < 8; ++j) av[j] = a[l * 8 + j];
  for (int j = 0; j < 4; ++j) bv[j] = b[l * 4 + j];
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, acc, 0, 4, OSA, sa[l], OSB, sb[l]);
  for (int r = 0; r < 4; ++r) out[l * 4 + r] = acc[r];
}

struct Dev { int *a, *b, *sa, *sb; float* out; };
static std::vector<int> A(512), Bv(256), SA(64), SB(64);
static float D[16][16];   // D[m][n]

static int run(Dev& d, int osa, int osb) {
  CK(hipMemcpy(d.a, A.data(), 2048, hipMemcpyHostToDevice));
  CK(hipMemcpy(d.b, Bv.data(), 1024, hipMemcpyHostToDevice));
  CK(hipMemcpy(d.sa, SA.data(), 256, hipMemcpyHostToDevice));
  CK(hipMemcpy(d.sb, SB.data(), 256, hipMemcpyHostToDevice));
  if (osa == 0 && osb == 0) probe<0, 0><<<1, 64>>>(d.a, d.b, d.sa, d.sb, d.out);
  else if (osa == 0 && osb == 1) probe<0, 1><<<1, 64>>>(d.a, d.b, d.sa, d.sb, d.out);
  else if (osa == 0 && osb == 2) probe<0, 2><<<1, 64>>>(d.a, d.b, d.sa, d.sb, d.out);
  else if (osa == 0 && osb == 3) probe<0, 3><<<1, 64>>>(d.a, d.b, d.sa, d.sb, d.out);
  else probe<1, 0><<<1, 64>>>(d.a, d.b, d.sa, d.sb, d.out);
  float o[256];
  CK(hipDeviceSynchronize());
  CK(hipMemcpy(o, d.out, 1024, hipMemcpyDeviceToHost));
  for (int l = 0; l < 64; ++l) for (int r = 0; r < 4; ++r) D[4 * (l >> 4) + r][l & 15] = o[l * 4 + r];
  return 0;
}
static void ones() {
  for (auto& v : A) v = 0x38383838;
  for (auto& v : Bv) v = 0x22222222;
  for (auto& v : SA) v = 0x7f7f7f7f;
  for (auto& v : SB) v = 0x7f7f7f7f;
}

int main() {
  Dev d;
  CK(hipMalloc(&d.a, 2048)); CK(hipMalloc(&d.b, 1024)); CK(hipMalloc(&d.sa, 256)); CK(hipMalloc(&d.sb, 256));
  CK(hipMalloc(&d.out, 1024));
  ones();
  if (run(d, 0, 0)) return 1;
  printf("all ones: D[0][0] = %g D[15][15] = %g (want 128)\n", D[0][0], D[15][15]);
  // 1. B scale: lane L's byte 0 = 128 -> column L & 15 gains 32 (block L >> 4 doubled)?
  int ok = 0;
  for (int L = 0; L < 64; ++L) {
    ones(); SB[L] = 0x7f7f7f80;
    if (run(d, 0, 0)) return 1;
    bool good = true;
    for (int m = 0; m < 16; ++m) for (int n = 0; n < 16; ++n) good &= D[m][n] == (n == (L & 15) ? 160.f : 128.f);
    ok += good;
    if (!good && L < 20) { printf("  B scale lane %d: row0:", L); for (int n = 0; n < 16; ++n) printf(" %g", D[0][n]); printf("\n"); }
  }
  printf("B scale lane (g, i) -> column i, one block of 32: %d / 64 lanes as expected\n", ok);
  // which block: A nonzero only in lane group G, lane L = 16 G' + 3 scaled: the gain is the overlap
  // of A group G's k with B's block G'
  for (int G = 0; G < 4; ++G) {
    printf("A only in lane group %d; B scale doubled in lane group g' = 0..3 of column 3: D[0][3] =", G);
    for (int Gp = 0; Gp < 4; ++Gp) {
      ones();
      for (int l = 0; l < 64; ++l) if ((l >> 4) != G) for (int j = 0; j < 8; ++j) A[l * 8 + j] = 0;
      SB[16 * Gp + 3] = 0x7f7f7f80;
      if (run(d, 0, 0)) return 1;
      printf(" %g", D[0][3]);
    }
    printf("  (48: half of A's 32 elements lie in B's block g')\n");
  }
  // 2. op_sel of B's scale: byte `by` of lane 5's scale register = 128
  for (int os = 0; os < 4; ++os) {
    printf("op_sel_b %d, the 128 in byte 0..3: D[0][5] =", os);
    for (int by = 0; by < 4; ++by) {
      ones(); SB[5] = 0x7f7f7f7f + (1 << (8 * by));
      if (run(d, 0, os)) return 1;
      printf(" %g", D[0][5]);
    }
    printf("\n");
  }
  // A's scale: lane 16 g + i -> row i
  ones(); SA[2 * 16 + 7] = 0x7f7f7f80;
  if (run(d, 0, 0)) return 1;
  printf("A scale lane (2, 7) doubled: D[7][0] = %g D[6][0] = %g (want 160, 128)\n", D[7][0], D[6][0]);
  // 3. k maps: A byte j of lane group g is k = 64 (j / 16) + 16 g + j % 16, B nibble j of lane
  //    group g is k = 32 g + j
  ok = 0;
  for (int k = 0; k < 128; ++k) {
    for (auto& v : A) v = 0; for (auto& v : Bv) v = 0;
    for (auto& v : SA) v = 0x7f7f7f7f; for (auto& v : SB) v = 0x7f7f7f7f;
    const int ga = (k % 64) / 16, ja = 16 * (k / 64) + k % 16, gb = k / 32, jb = k % 32;
    for (int i = 0; i < 16; ++i) {
      A[(16 * ga + i) * 8 + ja / 4] = 0x38 << (8 * (ja & 3));
      Bv[(16 * gb + i) * 4 + jb / 8] = 2 << (4 * (jb & 7));
    }
    if (run(d, 0, 0)) return 1;
    bool good = true;
    for (int m = 0; m < 16; ++m) for (int n = 0; n < 16; ++n) good &= D[m][n] == 1.f;
    ok += good;
  }
  printf("k maps (A: 64 (j / 16) + 16 g + j %% 16, B: 32 g + j): %d / 128\n", ok);
  // 4. rows and columns: A only lane i = 4 (all g), B only lane i = 9
  ones();
  for (int l = 0; l < 64; ++l) {
    if ((l & 15) != 4) for (int j = 0; j < 8; ++j) A[l * 8 + j] = 0;
    if ((l & 15) != 9) for (int j = 0; j < 4; ++j) Bv[l * 4 + j] = 0;
  }
  if (run(d, 0, 0)) return 1;
  int nz = 0;
  for (int m = 0; m < 16; ++m) for (int n = 0; n < 16; ++n) nz += D[m][n] != 0;
  printf("A lane i = 4, B lane i = 9: D[4][9] = %g, nonzeros %d (want 128, 1)\n", D[4][9], nz);
  // 5. E4M3 bytes of 0 .. 15 and 16 n, and E2M1 codes
  const int lo[16] = {0x00, 0x38, 0x40, 0x44, 0x48, 0x4A, 0x4C, 0x4E, 0x50, 0x51, 0x52, 0x53, 0x54, 0x55, 0x56, 0x57};
  ok = 0;
  for (int n = 0; n < 16; ++n) for (int hi = 0; hi < 2; ++hi) {
    for (auto& v : A) v = 0; for (auto& v : Bv) v = 0;
    for (auto& v : SA) v = 0x7f7f7f7f; for (auto& v : SB) v = 0x7f7f7f7f;
    A[0] = n ? lo[n] + 0x20 * hi : 0; Bv[0] = 2;
    if (run(d, 0, 0)) return 1;
    ok += D[0][0] == (float)(hi ? 16 * n : n);
  }
  printf("E4M3 table entries: %d / 32\n", ok);
  const float grid[8] = {0, .5f, 1, 1.5f, 2, 3, 4, 6};
  ok = 0;
  for (int c = 0; c < 16; ++c) {
    for (auto& v : A) v = 0; for (auto& v : Bv) v = 0;
    A[0] = 0x38; Bv[0] = c;
    if (run(d, 0, 0)) return 1;
    ok += D[0][0] == ((c & 8) ? -grid[c & 7] : grid[c & 7]);
  }
  printf("E2M1 codes: %d / 16\n", ok);
  return 0;
}
