// Host driver of the two byte-frame laws of csrc/frame_bytes.h (no HIP), for tests/test_frame_bytes_cpu.py.  Raw little-endian data
// on stdin / stdout, so that no digit is lost to text:
//   frame_bytes_host unit     writes the 256 fp32 values frame_byte_to_unit(0) .. frame_byte_to_unit(255)
//   frame_bytes_host byte     reads fp32 values from stdin until it ends, writes frame_unit_to_byte of each, one byte per value
#include <cstdio>
#include <cstring>
#include <vector>

#include "../world_modelz_amd/csrc/frame_bytes.h"

static_assert(sizeof(float) == 4, "fp32");

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "unit")) {
    float u[256];
    for (unsigned b = 0; b < 256; ++b) u[b] = frame_byte_to_unit(b);
    return std::fwrite(u, sizeof(float), 256, stdout) == 256 ? 0 : 1;
  }
  if (argc == 2 && !std::strcmp(argv[1], "byte")) {
    std::vector<float> in(1 << 16);
    std::vector<unsigned char> out(in.size());
    for (;;) {
      const size_t n = std::fread(in.data(), sizeof(float), in.size(), stdin);
      if (n == 0) break;
      for (size_t i = 0; i < n; ++i) out[i] = frame_unit_to_byte(in[i]);
      if (std::fwrite(out.data(), 1, n, stdout) != n) return 1;
    }
    return std::ferror(stdin) ? 1 : 0;
  }
  std::fprintf(stderr, "usage: frame_bytes_host unit | byte\n");
  return 2;
}
