// train_host.cpp — the host side of the training additions, stand-alone (its own main, no device code; built by
// tests/test_train_ref.py with -fsanitize=address,undefined from this file, ply.cpp and image_decode.cpp).
//
//   train_host init <case> <out>   ptgs_gaussians_checkpoint_init's arithmetic (csrc/splat_train_math.h, what the
//                                  kernel calls per element) on a case file: u32 n, degree, in_place; then scales
//                                  3n, opacities n, colors 3n (f32). Writes log_scales 3n, logits n, sh n ROW.
//   train_host mse <case> <out>    ptgs_image_mse's term (train_sq_err) summed in index order: u32 pixels, channels;
//                                  image 4 pixels, target channels pixels. Writes one double.
//   train_host ply <dir>           ptgs_write_gaussian_ply -> ptgs_read_gaussian_ply, bit for bit, for degrees 0..3
//                                  and counts 0, 1, 1000 (NaN and Inf payloads included), and the error codes.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ptgs/ptgs.h"
#include "../../include/ptgs/ptgs_host.h"
#include "splat_train_math.h"

namespace {

bool read_all(const char* path, std::vector<uint8_t>& b) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  std::fseek(f, 0, SEEK_END);
  const long n = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  b.resize((size_t)n);
  const bool ok = std::fread(b.data(), 1, b.size(), f) == b.size();
  std::fclose(f);
  return ok;
}

bool write_all(const char* path, const void* p, size_t n) {
  FILE* f = std::fopen(path, "wb");
  if (!f) return false;
  const bool ok = std::fwrite(p, 1, n, f) == n;
  return std::fclose(f) == 0 && ok;
}

int run_init(const char* in, const char* out) {
  std::vector<uint8_t> b;
  if (!read_all(in, b) || b.size() < 12) return 2;
  uint32_t hdr[3];
  memcpy(hdr, b.data(), 12);
  const size_t n = hdr[0], deg = hdr[1], row = 3 * (deg + 1) * (deg + 1);
  if (deg > 3 || b.size() != 12 + 7 * n * 4) return 2;
  std::vector<float> scales(3 * n), opac(n), colors(3 * n);
  memcpy(scales.data(), b.data() + 12, 12 * n);
  memcpy(opac.data(), b.data() + 12 + 12 * n, 4 * n);
  memcpy(colors.data(), b.data() + 12 + 16 * n, 12 * n);
  std::vector<float> ls_buf(3 * n), lo_buf(n), sh(n * row);
  // in place: the outputs are the inputs' own arrays, as the kernel allows
  float* ls = hdr[2] ? scales.data() : ls_buf.data();
  float* lo = hdr[2] ? opac.data() : lo_buf.data();
  for (size_t e = 0; e < 3 * n; ++e) ls[e] = ptgs::train_log_scale(scales[e]);
  for (size_t i = 0; i < n; ++i) lo[i] = ptgs::train_logit(opac[i]);
  for (size_t j = 0; j < n * row; ++j) sh[j] = ptgs::train_sh_element(&colors[3 * (j / row)], (uint32_t)(j % row));
  std::vector<uint8_t> o((4 * n + n * row) * 4);
  memcpy(o.data(), ls, 12 * n);
  memcpy(o.data() + 12 * n, lo, 4 * n);
  memcpy(o.data() + 16 * n, sh.data(), 4 * n * row);
  return write_all(out, o.data(), o.size()) ? 0 : 2;
}

int run_mse(const char* in, const char* out) {
  std::vector<uint8_t> b;
  if (!read_all(in, b) || b.size() < 8) return 2;
  uint32_t hdr[2];
  memcpy(hdr, b.data(), 8);
  const size_t px = hdr[0], ch = hdr[1];
  if ((ch != 3 && ch != 4) || b.size() != 8 + (4 + ch) * px * 4) return 2;
  std::vector<float> a(4 * px), t(ch * px);
  memcpy(a.data(), b.data() + 8, 16 * px);
  memcpy(t.data(), b.data() + 8 + 16 * px, 4 * ch * px);
  double sum = 0.0;
  for (size_t p = 0; p < px; ++p)
    for (size_t c = 0; c < 3; ++c) sum += ptgs::train_sq_err(a[4 * p + c], t[ch * p + c]);
  return write_all(out, &sum, sizeof(sum)) ? 0 : 2;
}

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "train_host: line %d: %s\n", __LINE__, #cond);  \
      return 1;                                                            \
    }                                                                      \
  } while (0)

// every float a distinct bit pattern (a counter scrambled), with a NaN, the infinities and -0 among them
void fill(std::vector<float>& v, uint32_t salt) {
  for (size_t i = 0; i < v.size(); ++i) {
    uint32_t u = (uint32_t)(i * 2654435761u) ^ (salt * 0x9E3779B9u);
    if ((u & 0x7F800000u) == 0x7F800000u) u &= ~0x40000000u;  // (the reader widens to double: a signalling NaN is quieted)
    if (i % 97 == 3) u = 0x7FC00001u;
    if (i % 97 == 5) u = 0x7F800000u;
    if (i % 97 == 7) u = 0xFF800000u;
    if (i % 97 == 9) u = 0x80000000u;
    memcpy(&v[i], &u, 4);
  }
}

int run_ply(const std::string& dir) {
  for (uint32_t deg = 0; deg <= 3; ++deg) {
    for (uint32_t n : {0u, 1u, 1000u}) {
      const size_t K = (deg + 1) * (deg + 1);
      std::vector<float> m(3 * n), ls(3 * n), rot(4 * n), lo(n), sh(n * K * 3);
      fill(m, 1 + deg), fill(ls, 11 + deg), fill(rot, 21 + deg), fill(lo, 31 + deg), fill(sh, 41 + deg);
      const std::string path = dir + "/rt_" + std::to_string(deg) + "_" + std::to_string(n) + ".ply";
      CHECK(ptgs_write_gaussian_ply(path.c_str(), m.data(), ls.data(), rot.data(), lo.data(), sh.data(), n, deg) ==
            PTGS_OK);
      uint32_t cnt = 77, d = 77;
      CHECK(ptgs_read_gaussian_ply(path.c_str(), nullptr, nullptr, nullptr, nullptr, nullptr, 0, &cnt, &d) == PTGS_OK);
      CHECK(cnt == n && d == deg);
      std::vector<float> m2(3 * n), ls2(3 * n), rot2(4 * n), lo2(n), sh2(n * K * 3);
      CHECK(ptgs_read_gaussian_ply(path.c_str(), m2.data(), ls2.data(), rot2.data(), lo2.data(), sh2.data(), n, &cnt,
                                   &d) == PTGS_OK);
      CHECK(n == 0 || (!memcmp(m.data(), m2.data(), 12 * n) && !memcmp(ls.data(), ls2.data(), 12 * n) &&
                       !memcmp(rot.data(), rot2.data(), 16 * n) && !memcmp(lo.data(), lo2.data(), 4 * n) &&
                       !memcmp(sh.data(), sh2.data(), 12 * n * K)));
    }
  }
  float one[48] = {0};
  const std::string ok = dir + "/e.ply";
  CHECK(ptgs_write_gaussian_ply(nullptr, one, one, one, one, one, 1, 0) == PTGS_EINVAL);
  CHECK(ptgs_write_gaussian_ply(ok.c_str(), one, one, one, one, one, 1, 4) == PTGS_EINVAL);
  CHECK(ptgs_write_gaussian_ply(ok.c_str(), nullptr, one, one, one, one, 1, 0) == PTGS_EINVAL);
  CHECK(ptgs_write_gaussian_ply(ok.c_str(), one, one, one, one, nullptr, 1, 0) == PTGS_EINVAL);
  CHECK(ptgs_write_gaussian_ply(ok.c_str(), nullptr, nullptr, nullptr, nullptr, nullptr, 0, 3) == PTGS_OK);
  CHECK(ptgs_write_gaussian_ply((dir + "/no_such_dir/x.ply").c_str(), one, one, one, one, one, 1, 0) == PTGS_EIO);
  std::printf("round trips ok\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "init")) return run_init(argv[2], argv[3]);
  if (argc == 4 && !strcmp(argv[1], "mse")) return run_mse(argv[2], argv[3]);
  if (argc == 3 && !strcmp(argv[1], "ply")) return run_ply(argv[2]);
  std::fprintf(stderr, "usage: train_host init|mse <case> <out> | ply <dir>\n");
  return 2;
}
