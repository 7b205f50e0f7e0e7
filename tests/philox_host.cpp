// Host driver of csrc/wmz_philox.h (no HIP): prints what the generator of the token corruption, the context draw and the samplers
// gives, for tests/test_philox_cpu.py to check against its own restatement of Philox4x32-10.
//   philox_host [b <index> <stream> <seed>]... [u <word>]...      (numbers in any base strtoull takes: 0x.. for hex)
// Per `b`: the four words of the block, hex, then the four [0, 1) values of philox4_unit as hex floats;  per `u`: the word's [0, 1)
// value as a hex float.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../world_modelz_amd/csrc/wmz_philox.h"

int main(int argc, char** argv) {
  for (int i = 1; i < argc;) {
    if (!std::strcmp(argv[i], "b") && i + 3 < argc) {
      const unsigned long long idx = std::strtoull(argv[i + 1], nullptr, 0), stream = std::strtoull(argv[i + 2], nullptr, 0),
                               seed = std::strtoull(argv[i + 3], nullptr, 0);
      unsigned c[4];
      float u[4];
      philox4(idx, stream, seed, c);
      philox4_unit(idx, stream, seed, u);
      std::printf("%08x %08x %08x %08x %a %a %a %a\n", c[0], c[1], c[2], c[3], (double)u[0], (double)u[1], (double)u[2], (double)u[3]);
      i += 4;
    } else if (!std::strcmp(argv[i], "u") && i + 1 < argc) {
      std::printf("%a\n", (double)philox_unit((unsigned)std::strtoull(argv[i + 1], nullptr, 0)));
      i += 2;
    } else {
      std::fprintf(stderr, "usage: philox_host [b <index> <stream> <seed>]... [u <word>]...\n");
      return 2;
    }
  }
  return 0;
}
