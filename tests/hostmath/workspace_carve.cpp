// TEST INFRASTRUCTURE (tests/test_cpu_workspace.py): a stand-alone driver of csrc/gd3d_workspace.h and of the two header-only carves
// built on it (csrc/simota_common.h, csrc/rpn_proposal_common.h), compiled under -fsanitize=address,undefined and run as a program
// on the CPU.  For every carve: the size is taken at address 0, a heap block of EXACTLY that many bytes is carved — at every
// misalignment 0..255 of its base under the self-aligning contract, at a 256-byte aligned base under the caller-aligned one — and
// every buffer is written in full, at the size the op documents for it.  A carve that outgrows its own size function writes past
// the block, which the address sanitizer stops; buffers that share a byte lose their tags.  Prints OK.
#define GD3D_HOST_TWIN 1
#include "../../mmdet3d-gaussian_amd/csrc/gd3d_workspace.h"
#include "../../mmdet3d-gaussian_amd/csrc/rpn_proposal_common.h"
#include "../../mmdet3d-gaussian_amd/csrc/simota_common.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct Buf {
  const char* name;
  const void* p;
  size_t bytes;
};

#define FAIL(...) do { std::printf(__VA_ARGS__); std::printf("\n"); return false; } while (0)

// every buffer 256-byte aligned and inside the block; written in full with a tag of its own, then read back: no two share a byte
static bool write_all(const char* what, char* block, size_t size, const std::vector<Buf>& bufs) {
  for (size_t i = 0; i < bufs.size(); ++i) {
    char* p = (char*)bufs[i].p;
    if (((uintptr_t)p & 255) != 0) FAIL("%s: %s is not 256-byte aligned", what, bufs[i].name);
    if (p < block || p + bufs[i].bytes > block + size) FAIL("%s: %s leaves the block", what, bufs[i].name);
    std::memset(p, (int)(i + 1), bufs[i].bytes);
  }
  for (size_t i = 0; i < bufs.size(); ++i)
    for (size_t k = 0; k < bufs[i].bytes; ++k)
      if (((const unsigned char*)bufs[i].p)[k] != (unsigned char)(i + 1)) FAIL("%s: %s shares a byte with a later buffer", what, bufs[i].name);
  return true;
}

// a block of exactly `size` bytes whose first byte lies `misalign` bytes past a multiple of 256; *owner is what to free
static char* block_at(size_t misalign, size_t size, void** owner) {
  if (posix_memalign(owner, 256, misalign + size) != 0) return nullptr;
  return (char*)*owner + misalign;
}

static bool carver_caller_aligned(size_t n) {
  auto carve = [n](void* base, std::vector<Buf>* bufs) {
    gd3d::Carver c(base, gd3d::Carver::CALLER_ALIGNED);
    int* a = c.take<int>(8);
    long long* b = c.take<long long>(n);
    char* none = c.take<char>(0);
    char* d = c.take<char>(n + 1);
    unsigned short* e = c.take<unsigned short>(3 * n);
    if (bufs != nullptr) *bufs = {{"a", a, 32}, {"b", b, 8 * n}, {"none", none, 0}, {"d", d, n + 1}, {"e", e, 6 * n}};
    return c.bytes();
  };
  const size_t size = carve(nullptr, nullptr);
  if (size % 256 != 0 || size != 256 + gd3d::up256(8 * n) + gd3d::up256(n + 1) + gd3d::up256(6 * n)) FAIL("carver: size %zu at n %zu", size, n);
  void* owner = nullptr;
  char* block = block_at(0, size, &owner);
  std::vector<Buf> bufs;
  bool ok = block != nullptr && carve(block, &bufs) == size && bufs[0].p == block && write_all("carver, caller-aligned", block, size, bufs);
  std::free(owner);
  return ok;
}

static bool carver_self_aligning(size_t n) {
  auto carve = [n](void* base, std::vector<Buf>* bufs) {
    gd3d::Carver c(base, gd3d::Carver::SELF_ALIGNING);
    float* a = c.take<float>(n);
    double* b = c.take<double>(n + 3);
    if (bufs != nullptr) *bufs = {{"a", a, 4 * n}, {"b", b, 8 * (n + 3)}};
    return c.bytes();
  };
  const size_t size = carve(nullptr, nullptr);
  if (size != gd3d::up256(4 * n) + gd3d::up256(8 * (n + 3)) + 256) FAIL("carver: size %zu at n %zu", size, n);
  for (size_t m = 0; m < 256; ++m) {
    void* owner = nullptr;
    char* block = block_at(m, size, &owner);
    std::vector<Buf> bufs;
    const bool ok = block != nullptr && carve(block, &bufs) == size && (char*)bufs[0].p == block + (256 - m) % 256 &&
                    write_all("carver, self-aligning", block, size, bufs);
    std::free(owner);
    if (!ok) FAIL("carver, self-aligning: n %zu, base misaligned by %zu", n, m);
  }
  return true;
}

// the buffers as include/gd3d.h and csrc/simota_common.h document them
static bool simota_carve(int64_t P, int32_t B, int32_t G_cap, int32_t K) {
  simota::Args a;
  const size_t size = simota::carve(a, nullptr, P, B, G_cap, K);
  const size_t matches = (size_t)B * G_cap * K;
  for (size_t m = 0; m < 256; ++m) {
    void* owner = nullptr;
    char* block = block_at(m, size, &owner);
    bool ok = block != nullptr && simota::carve(a, block, P, B, G_cap, K) == size;
    ok = ok && write_all("simota", block, size,
                         {{"cand_cnt", a.cand_cnt, 4 * (size_t)B}, {"cand", a.cand, 4 * (size_t)P}, {"match_prior", a.match_prior, 4 * matches},
                          {"match_iou", a.match_iou, 4 * matches}, {"conflict", a.conflict, 4 * matches}});
    std::free(owner);
    if (!ok) FAIL("simota: P %lld B %d G_cap %d K %d, base misaligned by %zu", (long long)P, B, G_cap, K, m);
  }
  return true;
}

// the buffers as csrc/rpn_proposal_common.h documents them; hist, nsurv and cnt are one block, first, that one fill clears
static bool rpn_carve(int B, int N, int cap, size_t nms_bytes) {
  rpn_proposal::Args a;
  a.p.B = B; a.p.N = N; a.p.cap = cap;
  const size_t size = rpn_proposal::carve(a, nullptr, nms_bytes).bytes;
  const size_t b = (size_t)B, bc = b * (size_t)cap;
  for (size_t m = 0; m < 256; ++m) {
    void* owner = nullptr;
    char* block = block_at(m, size, &owner);
    if (block == nullptr) return false;
    const rpn_proposal::Carved w = rpn_proposal::carve(a, block, nms_bytes);
    const size_t hist_bytes = b * rpn_proposal::LEVELS * rpn_proposal::BINS * 4;
    bool ok = w.bytes == size && a.nblk == (N + rpn_proposal::SPAN - 1) / rpn_proposal::SPAN;
    ok = ok && (char*)a.hist == block + (256 - m) % 256 && (char*)a.nsurv == (char*)a.hist + gd3d::up256(hist_bytes) &&
         (char*)a.cnt == (char*)a.nsurv + gd3d::up256(4 * b) && (char*)a.hist + w.zero_bytes == (char*)a.cnt + gd3d::up256(4 * b) &&
         (char*)a.keys == (char*)a.hist + w.zero_bytes;
    ok = ok && write_all("rpn_proposal", block, size,
                         {{"hist", a.hist, hist_bytes}, {"nsurv", a.nsurv, 4 * b}, {"cnt", a.cnt, 4 * b}, {"keys", a.keys, 4 * b * (size_t)N},
                          {"tiecnt", a.tiecnt, 4 * b * (size_t)a.nblk}, {"surv", a.surv, 8 * bc}, {"sel", a.sel, 4 * bc}, {"box7", a.box7, 28 * bc},
                          {"bev5", a.bev5, 20 * bc}, {"score", a.score, 4 * bc}, {"label", a.label, 4 * bc}, {"dir", a.dir, 4 * bc},
                          {"order", a.order, 8 * bc}, {"thresh", a.thresh, 4 * b}, {"keep", a.keep, 8 * bc}, {"num_keep", a.num_keep, 8 * b},
                          {"nms", w.nms, nms_bytes}});
    std::free(owner);
    if (!ok) FAIL("rpn_proposal: B %d N %d cap %d nms %zu, base misaligned by %zu", B, N, cap, nms_bytes, m);
  }
  return true;
}

int main() {
  bool ok = true;
  for (size_t n : {(size_t)1, (size_t)32, (size_t)85, (size_t)1000}) ok = ok && carver_caller_aligned(n) && carver_self_aligning(n);
  ok = ok && simota_carve(300, 1, 5, 10) && simota_carve(0, 3, 0, 1) && simota_carve(4097, 4, 9, 32);
  ok = ok && rpn_carve(1, 70, 70, 1000) && rpn_carve(2, 2 * 4096 + 1, 100, 0) && rpn_carve(3, 4096, 64, 12345);
  std::printf(ok ? "OK\n" : "FAILED\n");
  return ok ? 0 : 1;
}
