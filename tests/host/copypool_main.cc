// copypool_main.cc -- the copy threads of the host pipeline (csrc/mifc_copypool.h) on their own: pools of 1, 2 and 4
// threads, two callers copying at the same time as the pipeline's feeder and drainer do, sizes around the 2 MiB slice,
// guard bytes on both sides of every buffer.  Exits non-zero on any mismatch.  Built by tests/test_hostpipe_cpu.py with
// plain g++, and by `make -C mi-fieldcalc_amd copypool-check` under the thread and the address sanitizers.
#include "mifc_copypool.h"

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

namespace {

const size_t MIB = size_t(1) << 20;
const size_t SIZES[] = {0, 1, 2 * MIB - 1, 2 * MIB, 2 * MIB + 1, 5 * MIB + 3};
const size_t NSIZES = sizeof SIZES / sizeof SIZES[0];
const size_t GUARD = 64;
const unsigned char GUARD_SRC = 0xA5, GUARD_DST = 0x5A, STALE = 0xEE;

std::atomic<int> g_errors(0);

void complain(const char* what, int threads, int caller, int round, size_t bytes, size_t at)
{
  if (g_errors.fetch_add(1) < 10)
    std::fprintf(stderr, "copypool: %s (pool of %d, caller %d, round %d, %zu bytes, offset %zu)\n", what, threads, caller, round, bytes, at);
}

inline unsigned char pattern(size_t i, unsigned seed)
{
  return (unsigned char)((i * 2654435761u + seed) >> 7);
}

// one caller: its own source and destination, both with guards; every size in turn, `rounds` times
void caller(mifc::CopyPool* pool, int threads, int who, int rounds)
{
  const size_t cap = SIZES[NSIZES - 1];
  std::vector<unsigned char> src(cap + 2 * GUARD, GUARD_SRC), dst(cap + 2 * GUARD, GUARD_DST);
  for (int r = 0; r < rounds; ++r) {
    const size_t bytes = SIZES[(size_t)(r + who) % NSIZES];
    const unsigned seed = (unsigned)(r * 31 + who * 7 + threads);
    for (size_t i = 0; i < bytes; ++i) {
      src[GUARD + i] = pattern(i, seed);
      dst[GUARD + i] = STALE;
    }
    pool->copy(dst.data() + GUARD, src.data() + GUARD, bytes);
    for (size_t i = 0; i < bytes; ++i)
      if (dst[GUARD + i] != pattern(i, seed) || src[GUARD + i] != pattern(i, seed)) {
        complain("content differs", threads, who, r, bytes, i);
        break;
      }
    for (size_t i = 0; i < GUARD; ++i) {
      if (dst[i] != GUARD_DST)
        complain("guard in front of the destination overwritten", threads, who, r, bytes, i);
      if (src[i] != GUARD_SRC || src[GUARD + cap + i] != GUARD_SRC)
        complain("guard of the source overwritten", threads, who, r, bytes, i);
      if (dst[GUARD + cap + i] != GUARD_DST)
        complain("guard behind the destination buffer overwritten", threads, who, r, bytes, i);
    }
    // the same copy again with guard bytes directly behind the copied range: a slice that runs past its end shows there
    for (size_t i = bytes; i < bytes + GUARD && i < cap; ++i)
      dst[GUARD + i] = GUARD_DST;
    if (bytes + GUARD <= cap) {
      pool->copy(dst.data() + GUARD, src.data() + GUARD, bytes);
      for (size_t i = bytes; i < bytes + GUARD; ++i)
        if (dst[GUARD + i] != GUARD_DST) {
          complain("byte behind the copied range overwritten", threads, who, r, bytes, i);
          break;
        }
      if (bytes && (dst[GUARD] != pattern(0, seed) || dst[GUARD + bytes - 1] != pattern(bytes - 1, seed)))
        complain("content differs after the second copy", threads, who, r, bytes, 0);
    }
  }
}

} // namespace

int main(int argc, char** argv)
{
  int rounds = 72; // per caller and pool: 2 x 3 x 72 = 432 rounds, two copies each
  if (argc > 1)
    rounds = std::atoi(argv[1]);
  const int pools[] = {1, 2, 4};
  for (int threads : pools) {
    mifc::CopyPool pool(threads);
    std::thread feeder(caller, &pool, threads, 0, rounds);
    std::thread drainer(caller, &pool, threads, 1, rounds);
    feeder.join();
    drainer.join();
    // the pool is idle here and is destroyed at the end of the block: its workers must leave their wait and join
  }
  {
    mifc::CopyPool unused(3); // created and destroyed without a single copy
  }
  if (g_errors.load()) {
    std::fprintf(stderr, "copypool: %d mismatches\n", g_errors.load());
    return 1;
  }
  std::printf("copypool ok: pools of 1, 2 and 4 threads, %d rounds per caller\n", rounds);
  return 0;
}
