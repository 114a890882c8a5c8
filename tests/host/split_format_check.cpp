// Host-side driver of adm_amd/csrc/split_format.h for tests/test_split_format_host.py: runs the header's scalar functions on the CPU
// and writes raw results to stdout.  Built host-only (hipcc -x hip --cuda-host-only); no GPU is touched.
//   scale  FILE          FILE = n float32 bounds             -> n float32: split_scale
//   split3 FILE          FILE = n float32 values             -> [3][n] uint16: split3_store with term stride n
//   split2 FILE S        the values times the float S        -> [2][n] uint16: split2_store with term stride n, then n bytes:
//                                                               split_f16_overflow of the scaled value
//   layout ROWS COLS T   T = terms                           -> int64 element offsets, term included: wino_image_offset in the order
//                                                               [ey][ex][term][n][c], then rows_image_offset in the order [term][n][c]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../adm_amd/csrc/split_format.h"

static std::vector<float> read_floats(const char* path) {
  std::vector<float> v;
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
  float buf[1024];
  size_t n;
  while ((n = fread(buf, sizeof(float), 1024, f)) > 0) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return v;
}

template <class T> static void put(const std::vector<T>& v) {
  if (fwrite(v.data(), sizeof(T), v.size(), stdout) != v.size()) exit(3);
}

int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "";
  if (!strcmp(mode, "scale") && argc == 3) {
    std::vector<float> v = read_floats(argv[2]);
    for (float& x : v) x = split_scale(x);
    put(v);
  } else if (!strcmp(mode, "split3") && argc == 3) {
    const std::vector<float> v = read_floats(argv[2]);
    const long n = (long)v.size();
    std::vector<unsigned short> t(3 * n);
    for (long i = 0; i < n; ++i) split3_store(v[i], t.data() + i, n);
    put(t);
  } else if (!strcmp(mode, "split2") && argc == 4) {
    const std::vector<float> v = read_floats(argv[2]);
    const float s = strtof(argv[3], nullptr);
    const long n = (long)v.size();
    std::vector<unsigned short> t(2 * n);
    std::vector<unsigned char> bad(n);
    for (long i = 0; i < n; ++i) {
      const float a = v[i] * s;
      split2_store(a, t.data() + i, n);
      bad[i] = split_f16_overflow(a) ? 1 : 0;
    }
    put(t);
    put(bad);
  } else if (!strcmp(mode, "layout") && argc == 5) {
    const int rows = atoi(argv[2]), cols = atoi(argv[3]), terms = atoi(argv[4]);
    std::vector<long> o;
    for (int ey = 0; ey < 4; ++ey)
      for (int ex = 0; ex < 4; ++ex)
        for (int t = 0; t < terms; ++t)
          for (int n = 0; n < rows; ++n)
            for (int c = 0; c < cols; ++c) o.push_back(wino_image_offset(terms, ey, ex, rows, cols, n, c) + t * split_term_stride(rows));
    for (int t = 0; t < terms; ++t)
      for (int n = 0; n < rows; ++n)
        for (int c = 0; c < cols; ++c) o.push_back(rows_image_offset(terms, rows, n, c) + t * split_term_stride(rows));
    put(o);
  } else {
    fprintf(stderr, "usage: %s scale FILE | split3 FILE | split2 FILE S | layout ROWS COLS TERMS\n", argv[0]);
    return 2;
  }
  return 0;
}
