// Host driver of the SH colour's backward (csrc/splat_sh_math.h), for tests/test_sh_grad_ref.py:
//   sh_backward_host IN OUT
// IN: u32 n, sh_degree, active_degree, in_place; camera_pos (3 floats); means (3 n), sh (n K 3), dL/d colour (3 n);
// OUT: dL/d sh (n K 3), then dL/d mean (3 n, added to zeros), then the forward's colours (3 n).
// in_place != 0: each row of dL/d sh is written over a copy of its coefficients, as the GPU kernel does in LDS.
// No device code.
#include <cstdio>
#include <vector>

#include "splat_sh_math.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  uint32_t hdr[4];
  float cam[3];
  if (fread(hdr, 4, 4, f) != 4 || fread(cam, 4, 3, f) != 3) return 4;
  const uint32_t n = hdr[0], deg = hdr[1], active = hdr[2], in_place = hdr[3];
  if (n > (1u << 24) || deg > 3 || active > deg) return 4;
  const size_t R = (size_t)ptgs::sh_row((int)deg);
  std::vector<float> means((size_t)n * 3), sh(n * R), dcol((size_t)n * 3);
  if (fread(means.data(), 4, means.size(), f) != means.size() || fread(sh.data(), 4, sh.size(), f) != sh.size() ||
      fread(dcol.data(), 4, dcol.size(), f) != dcol.size())
    return 4;
  fclose(f);
  std::vector<float> dsh(n * R), dmeans((size_t)n * 3, 0.0f), colors((size_t)n * 3);
  const ptgs::v3 c = ptgs::mk3(cam[0], cam[1], cam[2]);
  for (uint32_t i = 0; i < n; ++i) {
    float len;
    const ptgs::v3 dir = ptgs::sh_dir(&means[(size_t)3 * i], c, &len);
    const float* row = &sh[i * R];
    switch (deg) {
      case 0: ptgs::sh_eval<0>(row, active, dir, &colors[(size_t)3 * i]); break;
      case 1: ptgs::sh_eval<1>(row, active, dir, &colors[(size_t)3 * i]); break;
      case 2: ptgs::sh_eval<2>(row, active, dir, &colors[(size_t)3 * i]); break;
      default: ptgs::sh_eval<3>(row, active, dir, &colors[(size_t)3 * i]); break;
    }
    float* drow = &dsh[i * R];
    if (in_place) {
      for (size_t j = 0; j < R; ++j) drow[j] = row[j];
      row = drow;
    }
    if (!ptgs::sh_backward_one_deg(deg, row, active, dir, len, &dcol[(size_t)3 * i], drow, &dmeans[(size_t)3 * i]))
      return 6;
  }
  f = fopen(argv[2], "wb");
  if (!f || fwrite(dsh.data(), 4, dsh.size(), f) != dsh.size() ||
      fwrite(dmeans.data(), 4, dmeans.size(), f) != dmeans.size() ||
      fwrite(colors.data(), 4, colors.size(), f) != colors.size())
    return 5;
  fclose(f);
  return 0;
}
