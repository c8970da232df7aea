// ring.h — the one host-side ring buffer of rows under the five on-device time series (monitor, modes, spectrum, hist,
// section).  A row is bytes: the owner knows what lies in it.  Row number n (counted since the arm) lives in slot n % capacity
// of the device allocation [header | capacity rows]; its labels (step, time) live in the host's vectors at the same slot.  Once
// more than `capacity` rows were recorded the oldest are overwritten: `held` rows can be read, `dropped` are gone.
#pragma once
#include <cstddef>
#include <cstdint>

namespace ekpnp {

// ---- index arithmetic: no HIP, includable by a plain C++ compiler (tests/ring_check.cpp)
struct RingPiece {
  int64_t slot, n;  // rows slot .. slot + n - 1 of the ring, contiguous
};
inline int64_t ring_held(int64_t recorded, int64_t capacity) { return recorded > capacity ? capacity : recorded; }
// may rows [first, first + count) of the held ones be read?
inline bool ring_range_ok(int64_t held, int64_t first, int64_t count) { return first >= 0 && count >= 0 && first + count <= held; }
// the slots of held rows [first, first + count), oldest first: at most two contiguous pieces (a valid range is assumed)
inline int ring_pieces(int64_t recorded, int64_t capacity, int64_t first, int64_t count, RingPiece piece[2]) {
  const int64_t seq0 = recorded - ring_held(recorded, capacity) + first;
  int np = 0;
  for (int64_t k = 0; k < count && np < 2;) {
    const int64_t slot = (seq0 + k) % capacity;
    const int64_t n = count - k < capacity - slot ? count - k : capacity - slot;
    piece[np++] = RingPiece{slot, n};
    k += n;
  }
  return np;
}

}  // namespace ekpnp

#if defined(__HIPCC__)
#include "ekpnp_internal.h"

namespace ekpnp {

struct Ring {
  void* alloc = nullptr;  // one allocation: [header | rows]
  size_t bytes = 0, row_bytes = 0, header_bytes = 0;
  int capacity = 0;
  int64_t recorded = 0;           // rows enqueued since the arm
  std::vector<int64_t> lab_step;  // the labels of the rows, [capacity]
  std::vector<double> lab_time;
  bool armed = false, ever_armed = false;
  char* rows() const { return (char*)alloc + header_bytes; }
};

// Disarm, wait for the stream (rows of an earlier arm may still be on their way into the ring), take a zeroed ring of this
// shape - the old allocation if its size is unchanged - and arm it.  Ctx::bytes follows; a failed allocation leaves no ring.
inline int ring_arm(Ctx& c, Ring& r, int capacity, size_t row_bytes, size_t header_bytes = 0) {
  r.armed = false;
  HIPCHK(c, hipStreamSynchronize(c.stream));
  const size_t bytes = header_bytes + (size_t)capacity * row_bytes;
  if (!r.alloc || r.bytes != bytes) {
    if (r.alloc) {
      (void)hipFree(r.alloc);
      c.bytes -= r.bytes;
      r.alloc = nullptr;
      r.bytes = 0;
    }
    HIPCHK(c, hipMalloc(&r.alloc, bytes));
    r.bytes = bytes;
    c.bytes += bytes;
  }
  HIPCHK(c, hipMemsetAsync(r.alloc, 0, bytes, c.stream));
  r.row_bytes = row_bytes;
  r.header_bytes = header_bytes;
  r.capacity = capacity;
  r.recorded = 0;
  r.lab_step.assign((size_t)capacity, 0);
  r.lab_time.assign((size_t)capacity, 0.0);
  r.armed = r.ever_armed = true;
  return EKPNP_OK;
}

inline size_t ring_next_slot(const Ring& r) { return (size_t)(r.recorded % r.capacity); }
// where the next row goes (device memory)
inline void* ring_next_row(const Ring& r) { return r.rows() + ring_next_slot(r) * r.row_bytes; }
// the next row has been enqueued: label it and count it
inline void ring_note_row(Ring& r, int64_t step, double time) {
  const size_t slot = ring_next_slot(r);
  r.lab_step[slot] = step;
  r.lab_time[slot] = time;
  ++r.recorded;
}

// no ring (never armed, or its allocation failed): 0 recorded, 0 dropped
inline void ring_count(const Ring* r, int64_t* recorded, int64_t* dropped) {
  const int64_t rec = r && r->alloc ? r->recorded : 0;
  if (recorded) *recorded = rec;
  if (dropped) *dropped = rec - (r && r->alloc ? ring_held(rec, r->capacity) : rec);
}

// held rows [first, first + count), oldest first, into rows ([count][row_bytes]) with their labels; waits for the stream
inline int ring_read(Ctx& c, const Ring* r, const char* who, int64_t first, int count, int64_t* steps, double* times, void* rows) {
  int64_t rec = 0, dropped = 0;
  ring_count(r, &rec, &dropped);
  const int64_t held = rec - dropped;
  if (!ring_range_ok(held, first, count)) {
    c.err = std::string(who) + ": rows " + std::to_string(first) + " .. " + std::to_string(first + (int64_t)count - 1) + " asked for, " + std::to_string(held) +
            " held";
    return EKPNP_ERR_INVALID;
  }
  if (count == 0) return EKPNP_OK;
  if (!steps || !times || !rows) return fail(c, "NULL pointer");
  HIPCHK(c, hipStreamSynchronize(c.stream));
  RingPiece piece[2];
  const int np = ring_pieces(rec, r->capacity, first, count, piece);
  for (int i = 0, k = 0; i < np; k += (int)piece[i++].n) {
    const size_t slot = (size_t)piece[i].slot, n = (size_t)piece[i].n;
    HIPCHK(c, hipMemcpy((char*)rows + (size_t)k * r->row_bytes, r->rows() + slot * r->row_bytes, n * r->row_bytes, hipMemcpyDeviceToHost));
    for (size_t j = 0; j < n; ++j) {
      steps[k + j] = r->lab_step[slot + j];
      times[k + j] = r->lab_time[slot + j];
    }
  }
  return EKPNP_OK;
}

inline void ring_release(Ring& r) {
  if (r.alloc) (void)hipFree(r.alloc);
  r.alloc = nullptr;
}

}  // namespace ekpnp
#endif
