// One-wave probe of v_smfmac_f32_16x16x64_bf16 (A 2:4-compressed, 8 bf16 per lane; B dense, 16 bf16
// per lane; a 32-bit index register): which B element each compressed A element meets at each
// 2-bit position, which index bits belong to which A element, and what cbsz / abid select
// (docs/kernels.md "2:4 sparse evaluation"; the recorded output is
// profiles/sparse24/instruction_probe.txt).  The dense k of an element is not observable, only
// which A element multiplies which B element, so the tables are printed as found.
// hipcc --offload-arch=gfx950 -O2 -o sp24_probe sp24_probe.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <vector>
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

// a, b: bf16 bit patterns, 8 and 16 per lane
template <int CBSZ, int ABID>
__global__ void probe(const uint16_t* a, const uint16_t* b, const int* idx, float* out) {
  const int l = threadIdx.x;
  uint16_t ar[8], br[16];
  for (int j = 0; j < 8; ++j) ar[j] = a[l * 8 + j];
  for (int j = 0; j < 16; ++j) br[j] = b[l * 16 + j];
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_smfmac_f32_16x16x64_bf16(__builtin_bit_cast(bf16x8, ar),
                                                  __builtin_bit_cast(bf16x16, br), acc, idx[l], CBSZ, ABID);
  for (int r = 0; r < 4; ++r) out[l * 4 + r] = acc[r];
}

struct Dev { uint16_t *a, *b; int* idx; float* out; };
static std::vector<uint16_t> A(512), Bv(1024);
static std::vector<int> IDX(64);
static float D[16][16];   // D[m][n], assuming the usual fragment: lane (g, i) holds D[4 g + r][i]
constexpr uint16_t ONE = 0x3F80;

static int run(Dev& d, int cbsz, int abid) {
  CK(hipMemcpy(d.a, A.data(), 1024, hipMemcpyHostToDevice));
  CK(hipMemcpy(d.b, Bv.data(), 2048, hipMemcpyHostToDevice));
  CK(hipMemcpy(d.idx, IDX.data(), 256, hipMemcpyHostToDevice));
  if (cbsz == 0 && abid == 0) probe<0, 0><<<1, 64>>>(d.a, d.b, d.idx, d.out);
  else if (cbsz == 0 && abid == 1) probe<0, 1><<<1, 64>>>(d.a, d.b, d.idx, d.out);
  else if (cbsz == 1 && abid == 0) probe<1, 0><<<1, 64>>>(d.a, d.b, d.idx, d.out);
  else probe<1, 1><<<1, 64>>>(d.a, d.b, d.idx, d.out);
  float o[256];
  CK(hipDeviceSynchronize());
  CK(hipMemcpy(o, d.out, 1024, hipMemcpyDeviceToHost));
  for (int l = 0; l < 64; ++l) for (int r = 0; r < 4; ++r) D[4 * (l >> 4) + r][l & 15] = o[l * 4 + r];
  return 0;
}
static void clear() {
  for (auto& v : A) v = 0;
  for (auto& v : Bv) v = 0;
  for (auto& v : IDX) v = 0;
}

int main() {
  Dev d;
  CK(hipMalloc(&d.a, 1024)); CK(hipMalloc(&d.b, 2048)); CK(hipMalloc(&d.idx, 256)); CK(hipMalloc(&d.out, 1024));
  // 0. rows and columns: A only in lanes i = 4 (all g), B only in lanes i = 9, everything 1,
  //    positions (0, 1) in every group: 32 products
  clear();
  for (int l = 0; l < 64; ++l) {
    if ((l & 15) == 4) for (int j = 0; j < 8; ++j) A[l * 8 + j] = ONE;
    if ((l & 15) == 9) for (int j = 0; j < 16; ++j) Bv[l * 16 + j] = ONE;
    IDX[l] = 0x44444444;
  }
  if (run(d, 0, 0)) return 1;
  int nz = 0;
  for (int m = 0; m < 16; ++m) for (int n = 0; n < 16; ++n) nz += D[m][n] != 0;
  printf("A lanes i = 4, B lanes i = 9: D[4][9] = %g, nonzeros %d (want 32, 1: A lane i is row i, B lane i column i)\n",
         D[4][9], nz);
  // 1. the meeting table: A element e of lane group ga, every index field at position p, meets
  //    which B element (gb, jb)?  16 B elements per launch, one per column.
  int meet[4][8][4];          // -> 16 gb + jb, -1 none, -2 several
  for (int ga = 0; ga < 4; ++ga) for (int e = 0; e < 8; ++e) for (int p = 0; p < 4; ++p) {
    int found = -1;
    for (int c = 0; c < 4; ++c) {
      clear();
      for (int i = 0; i < 16; ++i) {
        A[(16 * ga + i) * 8 + e] = ONE;
        const int t = 16 * c + i;                   // column i tests B element t
        Bv[(16 * (t >> 4) + i) * 16 + (t & 15)] = ONE;
      }
      for (auto& v : IDX) v = p * 0x55555555;
      if (run(d, 0, 0)) return 1;
      for (int i = 0; i < 16; ++i) if (D[0][i] != 0) found = found == -1 ? 16 * c + i : -2;
    }
    meet[ga][e][p] = found;
  }
  int same_g = 0, aligned = 0;
  for (int ga = 0; ga < 4; ++ga) {
    printf("A lane group %d, element e: B (lane group, element) met at position 0..3\n", ga);
    for (int e = 0; e < 8; ++e) {
      printf("  e = %d:", e);
      for (int p = 0; p < 4; ++p) {
        const int t = meet[ga][e][p];
        if (t < 0) printf(" (none %d)", t); else printf(" (%d, %2d)", t >> 4, t & 15);
        same_g += t >= 0 && (t >> 4) == ga;
        aligned += t >= 0 && (t & 15) == 4 * (e >> 1) + p;
      }
      printf("\n");
    }
  }
  printf("same lane group: %d / 128, B element = 4 (e / 2) + p: %d / 128\n", same_g, aligned);
  // 2. the index fields: lane (ga, m) has 3 in field m alone, its element e is 1, every column's
  //    B is the element met at position 3: row m answers iff field m places element e
  for (int cbsz = 0; cbsz < 2; ++cbsz) for (int abid = 0; abid < 2; ++abid) {
    printf("cbsz %d abid %d, 2-bit field of element e (lane group 0 | 1 | 2 | 3):", cbsz, abid);
    for (int e = 0; e < 8; ++e) {
      printf(" e%d", e);
      for (int ga = 0; ga < 4; ++ga) {
        const int t = meet[ga][e][3];
        if (t < 0) { printf(" ?"); continue; }
        clear();
        for (int i = 0; i < 16; ++i) {
          A[(16 * ga + i) * 8 + e] = ONE;
          IDX[16 * ga + i] = 3 << (2 * i);
          Bv[(16 * (t >> 4) + i) * 16 + (t & 15)] = ONE;
        }
        if (run(d, cbsz, abid)) return 1;
        int f = -1;
        for (int m = 0; m < 16; ++m) if (D[m][0] != 0) f = f == -1 ? m : -2;
        printf("%c%d", ga ? '|' : ' ', f);
      }
    }
    printf("\n");
  }
  // 3. does a lane's index come from its own register?  lane (1, 5) alone has positions (2, 3)
  clear();
  for (auto& v : A) v = ONE;
  for (int l = 0; l < 64; ++l) IDX[l] = 0x44444444;
  IDX[16 + 5] = (int)0xEEEEEEEE;
  for (int l = 0; l < 64; ++l) for (int j = 0; j < 16; ++j) Bv[l * 16 + j] = (j & 2) ? 0x4000 : ONE;   // 1 1 2 2
  if (run(d, 0, 0)) return 1;
  printf("own index: D[5][0] = %g D[4][0] = %g (want 40 = 24 + 16 and 32)\n", D[5][0], D[4][0]);
  return 0;
}
