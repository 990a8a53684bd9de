// gsply_fuzz.cpp — ptgs_read_gaussian_ply (and ptgs_read_ply on the same files) under AddressSanitizer +
// UndefinedBehaviorSanitizer: a stand-alone driver (no device code; the sanitizer runtimes are linked
// in), built and run by tests/test_gaussian_ply_sanitize.py.
//
//   gsply_fuzz <scratch dir> <mutations per seed file> [rng seed]
//
// It writes a valid trained-3DGS checkpoint of every degree 0..3 in every format (ascii, binary little
// and big endian) into the scratch directory, loads each and checks what comes back, then loads
// deterministic mutations of each: numbers in the header replaced, property lines deleted or
// duplicated, the file truncated, bytes flipped. A mutated file may be accepted or rejected; a
// sanitizer report or an abort ends the process with a non-zero status.
#include <sys/stat.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ptgs/ptgs_host.h"

namespace {

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // splitmix64
  uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
uint64_t rnd(uint64_t n) { return n ? rnd() % n : 0; }

void die(const char* what, const std::string& where) {
  fprintf(stderr, "gsply_fuzz: %s (%s)\n", what, where.c_str());
  exit(1);
}

void write_file(const std::string& p, const std::string& v) {
  FILE* f = fopen(p.c_str(), "wb");
  if (!f) die("cannot write", p);
  if (!v.empty() && fwrite(v.data(), 1, v.size(), f) != v.size()) die("short write", p);
  fclose(f);
}

const uint32_t kCount = 19;

std::vector<std::string> prop_names(int deg) {
  std::vector<std::string> n = {"x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"};
  for (int j = 0; j < 3 * ((deg + 1) * (deg + 1) - 1); ++j) n.push_back("f_rest_" + std::to_string(j));
  for (const char* s : {"opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"}) n.push_back(s);
  return n;
}

// value of property p of vertex i: exactly representable, different everywhere
float value(uint32_t i, size_t p) { return (float)((int)(i * 64 + p) - 300) * 0.125f; }

// fmt: 0 ascii, 1 little endian, 2 big endian. header_end: where the body starts.
std::string make_checkpoint(int deg, int fmt, size_t* header_end) {
  const std::vector<std::string> names = prop_names(deg);
  const char* fmts[3] = {"ascii", "binary_little_endian", "binary_big_endian"};
  std::string s = std::string("ply\nformat ") + fmts[fmt] + " 1.0\nelement vertex " + std::to_string(kCount) + "\n";
  for (const std::string& n : names) s += "property float " + n + "\n";
  s += "end_header\n";
  *header_end = s.size();
  for (uint32_t i = 0; i < kCount; ++i) {
    for (size_t p = 0; p < names.size(); ++p) {
      const float v = value(i, p);
      if (fmt == 0) {
        char buf[48];
        snprintf(buf, sizeof buf, "%.9g%c", v, p + 1 == names.size() ? '\n' : ' ');
        s += buf;
      } else {
        uint8_t b[4];
        memcpy(b, &v, 4);  // (the host is little endian)
        for (int k = 0; k < 4; ++k) s.push_back((char)b[fmt == 2 ? 3 - k : k]);
      }
    }
  }
  return s;
}

struct Loaded {
  int rc = 0;
  uint32_t count = 0, degree = 0;
  std::vector<float> means, scales, rots, opac, sh;
};

// query, then a full read into buffers sized from the query; both through the C-ABI
Loaded load(const std::string& path) {
  Loaded L;
  L.rc = ptgs_read_gaussian_ply(path.c_str(), nullptr, nullptr, nullptr, nullptr, nullptr, 0, &L.count, &L.degree);
  if (L.rc != PTGS_OK) return L;
  if (L.degree > 3) die("query returned a degree above 3", path);
  const size_t n = L.count, K = (size_t)(L.degree + 1) * (L.degree + 1);
  L.means.assign(n * 3, 0.f);
  L.scales.assign(n * 3, 0.f);
  L.rots.assign(n * 4, 0.f);
  L.opac.assign(n, 0.f);
  L.sh.assign(n * K * 3, 0.f);
  uint32_t c2 = 0, d2 = 0;
  L.rc = ptgs_read_gaussian_ply(path.c_str(), L.means.data(), L.scales.data(), L.rots.data(), L.opac.data(),
                                L.sh.data(), L.count, &c2, &d2);
  if (L.rc == PTGS_OK && (c2 != L.count || d2 != L.degree)) die("full read disagrees with the query", path);
  // partial outputs and a capacity one short
  if (n) {
    const int rc = ptgs_read_gaussian_ply(path.c_str(), nullptr, nullptr, nullptr, nullptr, L.sh.data(), L.count - 1,
                                          &c2, &d2);
    if (rc != PTGS_ERANGE) die("capacity below the count was not PTGS_ERANGE", path);
    (void)ptgs_read_gaussian_ply(path.c_str(), L.means.data(), nullptr, nullptr, L.opac.data(), nullptr, L.count, &c2,
                                 &d2);
  }
  return L;
}

void load_points(const std::string& path) {  // ptgs_read_ply shares the parser
  uint32_t n = 0;
  if (ptgs_read_ply(path.c_str(), nullptr, nullptr, nullptr, 0, &n) != PTGS_OK) return;
  std::vector<float> xyz((size_t)n * 3), nrm((size_t)n * 3);
  std::vector<uint8_t> rgb((size_t)n * 3);
  (void)ptgs_read_ply(path.c_str(), xyz.data(), nrm.data(), rgb.data(), n, &n);
}

void check_valid(const Loaded& L, int deg, const std::string& path) {
  if (L.rc != PTGS_OK || L.count != kCount || (int)L.degree != deg) die("valid checkpoint not loaded", path);
  const std::vector<std::string> names = prop_names(deg);
  const size_t K = (size_t)(deg + 1) * (deg + 1), rest0 = 9, tail = 9 + 3 * (K - 1);
  for (uint32_t i = 0; i < kCount; ++i) {
    bool ok = true;
    for (size_t a = 0; a < 3; ++a) ok &= L.means[3 * i + a] == value(i, a) && L.scales[3 * i + a] == value(i, tail + 1 + a);
    for (size_t a = 0; a < 4; ++a) ok &= L.rots[4 * i + a] == value(i, tail + 4 + a);
    ok &= L.opac[i] == value(i, tail);
    for (size_t c = 0; c < 3; ++c) {
      ok &= L.sh[(i * K) * 3 + c] == value(i, 6 + c);
      for (size_t k = 1; k < K; ++k) ok &= L.sh[(i * K + k) * 3 + c] == value(i, rest0 + c * (K - 1) + (k - 1));
    }
    if (!ok) die("valid checkpoint read back wrong", path);
  }
}

std::vector<std::pair<size_t, size_t>> header_lines(const std::string& s, size_t header_end) {
  std::vector<std::pair<size_t, size_t>> lines;  // [begin, end) with the newline
  for (size_t b = 0; b < header_end;) {
    size_t e = s.find('\n', b);
    e = e == std::string::npos ? header_end : e + 1;
    lines.push_back({b, e});
    b = e;
  }
  return lines;
}

std::string mutate(const std::string& seed, size_t header_end, bool text) {
  std::string s = seed;
  const auto lines = header_lines(s, header_end);
  switch (rnd(6)) {
    case 0: {  // a number of the header replaced (the vertex count, an f_rest_ / rot_ / scale_ index)
      std::vector<size_t> digits;
      for (size_t i = 0; i < header_end; ++i)
        if (s[i] >= '0' && s[i] <= '9' && (i == 0 || s[i - 1] < '0' || s[i - 1] > '9')) digits.push_back(i);
      if (digits.empty()) break;
      const size_t b = digits[rnd(digits.size())];
      size_t e = b;
      while (e < s.size() && s[e] >= '0' && s[e] <= '9') ++e;
      const char* subs[] = {"0", "1", "3", "44", "45", "46", "99", "4294967295", "4294967296", "18446744073709551615",
                            "-1", "007", "1e9", ""};
      s.replace(b, e - b, subs[rnd(sizeof subs / sizeof subs[0])]);
      break;
    }
    case 1: {  // a property (header line) deleted
      const auto& l = lines[rnd(lines.size())];
      s.erase(l.first, l.second - l.first);
      break;
    }
    case 2: {  // a property duplicated, in place or at the end of the property list
      const auto& l = lines[rnd(lines.size())];
      const std::string dup = s.substr(l.first, l.second - l.first);
      s.insert(rnd(2) ? l.first : lines.back().first, dup);
      break;
    }
    case 3:  // truncated, anywhere
      s.resize(rnd(s.size() + 1));
      break;
    case 4: {  // truncated inside the body, or a few bytes more
      if (rnd(2)) s.resize(header_end + rnd(s.size() - header_end + 1));
      else s.append(1 + rnd(7), text ? '1' : '\x7f');
      break;
    }
    default: {  // byte flips
      if (s.empty()) break;
      for (int k = 1 + (int)rnd(4); k > 0; --k) {
        const size_t i = rnd(2) ? rnd(s.size()) : rnd(header_end);
        s[i] = text && rnd(2) ? "0123456789 -.e\nx"[rnd(16)] : (char)(s[i] ^ (1u << rnd(8)));
      }
      break;
    }
  }
  return s;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s <scratch dir> <mutations per seed file> [rng seed]\n", argv[0]);
    return 2;
  }
  const std::string tmp = argv[1];
  const int M = atoi(argv[2]);
  if (argc > 3) g_rng ^= strtoull(argv[3], nullptr, 10) * 0xD1B54A32D192ED03ull;
  mkdir(tmp.c_str(), 0755);
  long runs = 0, accepted = 0;
  for (int deg = 0; deg <= 3; ++deg)
    for (int fmt = 0; fmt < 3; ++fmt) {
      size_t header_end = 0;
      const std::string seed = make_checkpoint(deg, fmt, &header_end);
      const std::string p = tmp + "/ckpt_d" + std::to_string(deg) + "_f" + std::to_string(fmt) + ".ply";
      write_file(p, seed);
      check_valid(load(p), deg, p);
      load_points(p);
      const std::string mp = tmp + "/mutated.ply";
      for (int k = 0; k < M; ++k, ++runs) {
        write_file(mp, mutate(seed, header_end, fmt == 0));
        accepted += load(mp).rc == PTGS_OK;
        load_points(mp);
      }
      remove(mp.c_str());
      remove(p.c_str());
    }
  // arguments
  uint32_t n = 0, d = 0;
  if (ptgs_read_gaussian_ply(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &n, &d) != PTGS_EINVAL ||
      ptgs_read_gaussian_ply("x", nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, &d) != PTGS_EINVAL ||
      ptgs_read_gaussian_ply((tmp + "/absent.ply").c_str(), nullptr, nullptr, nullptr, nullptr, nullptr, 0, &n, &d) !=
          PTGS_EIO)
    die("argument errors", "null / absent path");
  printf("gsply_fuzz: %ld mutated files (%ld accepted), no sanitizer report\n", runs, accepted);
  return 0;
}
