// ring_check.cpp — the index arithmetic of csrc/ring.h against a brute-force model (tests/test_ring_cpu.py builds and runs it).
// The model is a std::deque of row numbers: a row is pushed at the back, and the front is popped once more than `capacity` are
// held.  Row number n lives in slot n % capacity.  Prints "ok <cases>" and returns 0, or the first mismatch and 1.
#include <cstdint>
#include <cstdio>
#include <deque>
#include <vector>

#include "../ek-pnp-3d_amd/csrc/ring.h"

using namespace ekpnp;

#define CHECK(cond, ...)                  \
  do {                                    \
    if (!(cond)) {                        \
      std::printf("FAILED " __VA_ARGS__); \
      std::printf(" [%s]\n", #cond);      \
      return 1;                           \
    }                                     \
  } while (0)

int main() {
  long cases = 0;
  for (int64_t capacity : {1, 2, 3, 5}) {
    std::deque<int64_t> model;
    for (int64_t recorded = 0; recorded <= 3 * capacity + 1; ++recorded) {
      if (recorded > 0) {  // row number recorded - 1 arrives
        model.push_back(recorded - 1);
        if ((int64_t)model.size() > capacity) model.pop_front();
      }
      const int64_t held = ring_held(recorded, capacity);
      CHECK(held == (int64_t)model.size(), "capacity %lld recorded %lld: held %lld", (long long)capacity, (long long)recorded, (long long)held);
      CHECK(recorded - held == (model.empty() ? recorded : model.front()), "capacity %lld recorded %lld: dropped", (long long)capacity, (long long)recorded);
      for (int64_t first = -1; first <= held + 1; ++first)
        for (int64_t count = -1; first + count <= held + 1; ++count) {
          ++cases;
          const bool want_ok = first >= 0 && count >= 0 && first + count <= (int64_t)model.size();
          CHECK(ring_range_ok(held, first, count) == want_ok, "capacity %lld recorded %lld first %lld count %lld: acceptance", (long long)capacity,
                (long long)recorded, (long long)first, (long long)count);
          if (!want_ok) continue;
          RingPiece piece[2] = {{-7, -7}, {-7, -7}};
          const int np = ring_pieces(recorded, capacity, first, count, piece);
          CHECK(np >= 0 && np <= 2, "capacity %lld recorded %lld first %lld count %lld: %d pieces", (long long)capacity, (long long)recorded, (long long)first,
                (long long)count, np);
          std::vector<int64_t> slots;
          for (int i = 0; i < np; ++i) {
            CHECK(piece[i].n >= 1 && piece[i].slot >= 0 && piece[i].slot + piece[i].n <= capacity,
                  "capacity %lld recorded %lld first %lld count %lld: piece %d = (%lld, %lld) leaves the ring", (long long)capacity, (long long)recorded,
                  (long long)first, (long long)count, i, (long long)piece[i].slot, (long long)piece[i].n);
            for (int64_t j = 0; j < piece[i].n; ++j) slots.push_back(piece[i].slot + j);
          }
          CHECK((int64_t)slots.size() == count, "capacity %lld recorded %lld first %lld count %lld: %zu rows named", (long long)capacity, (long long)recorded,
                (long long)first, (long long)count, slots.size());
          for (int64_t k = 0; k < count; ++k)
            CHECK(slots[(size_t)k] == model[(size_t)(first + k)] % capacity, "capacity %lld recorded %lld first %lld count %lld: row %lld in slot %lld",
                  (long long)capacity, (long long)recorded, (long long)first, (long long)count, (long long)k, (long long)slots[(size_t)k]);
        }
    }
  }
  std::printf("ok %ld\n", cases);
  return 0;
}
