// ws_relax_queue.hpp -- the tile lists and the tile queue of the relaxation's late passes (ws_relax.hip): the layout of
// tile_list, the coherent stamp accesses of the queue pass, and the queue's protocols as device functions.
//
// PERSIST (the first same-grid pass of a long-range flood, relax_pass): ONE launch instead of a pass per step of the flood
// front.  The workgroups -- all resident -- pull tiles from a queue; a tile run that changes a side that matters to a
// neighbour, or stops at its round cap, puts that neighbour (itself) back into the queue, at once: no pass barrier, so the
// critical path is the chain of tile runs along the flood instead of the slowest tile of each of ~180 launches.
//   queue   a ring of (sequence number, tile) pairs in the two entry arrays of tile_list; head = the ticket word, tail = the
//           length word of this pass; a worker draws a ticket and waits for ITS entry (the sequence number tells it from the
//           ring's previous lap);
//   state   one word per tile (the "queued" marks): bit 0 queued -- or, while bit 1 is set, "flagged again while running" --,
//           bit 1 running.  A tile is in the queue at most once, and a tile flagged while it runs queues itself when it ends;
//   end     [RLQ_PENDING] counts tiles queued or running; who brings it to zero raises [RLQ_DONE].
// Exactness does not rest on any of this: stamps only ever fall, by relaxation steps from upper bounds (a stale read is an
// older, larger stamp: less progress, never a wrong value), and the pass AFTER this launch runs every tile once from an
// all-tiles list -- the flood is at its fixpoint when the ordinary passes that follow say so.
// What does rest on it is the launch's speed and its end: the order of the memory operations, waits, barriers and atomics
// in the functions below is part of the protocol.
#pragma once

#include "ws_relax_patch.hpp"      // u32x4_t

namespace wsk {

constexpr uint32_t RX_CAND = 64;      // candidates a workgroup collects before it hands them in (k_relax, append_flush)
// tile_list: [0 .. 3] list lengths and [4 .. 7] entry tickets of pass & 3 (a launch clears the words of pass + 2); from
// [RL_HDR] on the entries of the even passes, then of the odd ones, then one "queued for pass" word per tile.
constexpr uint32_t RL_HDR = 192;
// ... and, for the persistent tile-queue pass (k_relax, PERSIST): [8] tiles queued or running, [9] "the queue has run dry" (1) or
// "a worker ran out of its time budget" (2), [10] tile runs (diagnostics)
constexpr uint32_t RLQ_PHASE = 16;      // -DWS_TUNING: ticks of thread 0 per phase of a tile run, summed (load, rounds, epilogue, hand-in)
// Every word that all workers hammer sits on a 128-byte line of its own: head, tail, pending and the end flag in ONE line
// were ~100 atomics and polls per microsecond on one L2 channel, and an atomic round trip took 3 us (a tile run 49 us
// instead of 15).
constexpr uint32_t RLQ_HEAD = 32, RLQ_TAIL = 64, RLQ_PENDING = 96, RLQ_DONE = 128;
constexpr uint32_t RLQ_RUNS = 10, RLQ_WAIT = 11, RLQ_LIFE = 12, RLQ_POLLS = 13;      // (11-13: all workers' waiting / life time in 10 ns ticks, polls)
// A worker gives up -- and tells the others to -- when the launch has lasted this long (s_memrealtime ticks of 10 ns): no spin
// of this kernel can outlive it, whatever goes wrong with the queue.  What is left undone is work for the passes that follow.
constexpr unsigned long long RLQ_BUDGET_TICKS = 5000000ull;      // 50 ms; a smooth 8192^2 map needs 3
// PERSIST == 2, the queue in flood order: a worker takes a tile from the LOWEST non-empty of PQ_B buckets; a tile's bucket is the
// level (>> pq_shift) of the smallest stamp waiting at its borders.  tools/sim_tile_schedule.c (SIM_QUEUE=prio): on an 8192^2
// map of correlation length 64 px first-come order needs 152 k tile runs, this order 87 k with 32 buckets (86 k with 256):
// a tile that waits until the flood below it has passed runs once on final borders instead of once per arrival.
//   state   one word per tile: bit 31 running; bits 0 .. 30 "a stamp of bucket b waits" (idle: 0).  A tile that is not running and
//           has bits set is queued: its bit is set in the bitmap of its lowest bucket;
//   bucket  a bitmap over the tiles (idempotent: no ring, no overflow, no lap) and a count of its set bits; the 31 counts and a
//           copy of the end flag share ONE 128-byte line, so that a worker's look at all of them is one memory request (a line
//           per count: 32 requests per look, and the idle workers' looks alone slowed every tile load from 4 us to 21).
//           A stale bit (its tile runs, or has run from a lower bucket) costs a failed claim or one idle run.
constexpr int PQ_B = 31;
constexpr uint32_t PQ_RUNNING = 0x80000000u;
constexpr uint32_t PQ_HDR = 32;      // the counts' line: [b] set bits of bucket b, [31] the end flag again
__host__ __device__ inline size_t pq_base(uint32_t list_cap) { return (RL_HDR + 3 * (size_t)list_cap + 64 + 31) & ~(size_t)31; }
__host__ __device__ inline uint32_t pq_words_per_bucket(uint32_t tiles) { return ((tiles + 31u) / 32u + 255u) & ~255u; }      // whole 1 KiB chunks: one load of a wave
__host__ __device__ inline uint32_t pq_shift_of(uint32_t max_level) { return 24u + (max_level >= 124u ? 3u : max_level >= 62u ? 2u : max_level >= 31u ? 1u : 0u); }

// Stamp accesses of the persistent pass: tiles hand their border pixels to each other INSIDE a launch, across CUs and XCDs,
// so every stamp is stored write-through and loaded past L1 at agent scope (global_store / global_load ... sc1;
// MI355X_MICROARCH.md, inter-workgroup visibility).  Inline assembly, because HIP's agent-scope atomic loads are 8 bytes at
// most and each is waited for on its own: 24 dependent round trips per lane and tile run (52 us per run against 12).  The
// loads are issued back to back and waited for ONCE (the wait's operands tie the loaded registers to it, so that no use
// can be scheduled in front of it).
__device__ __forceinline__ void coh_load4(u32x4_t &v, const uint32_t *p) {
  asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(v) : "v"(p) : "memory");
}
__device__ __forceinline__ void coh_load1(uint32_t &v, const uint32_t *p) {
  asm volatile("global_load_dword %0, %1, off sc1" : "=v"(v) : "v"(p) : "memory");
}
__device__ __forceinline__ void coh_store4(uint32_t *p, u32x4_t v) {
  asm volatile("global_store_dwordx4 %0, %1, off sc1" : : "v"(p), "v"(v) : "memory");
}

// tile_list, the capacity of its entry arrays, and where the queue's words live in it (kernel uniform).  (When the launch
// began, and a worker's waiting time and looks, stay locals of k_relax and are passed to the take functions.)
struct RelaxQueue {
  uint32_t *tile_list;
  uint32_t list_cap;
  unsigned long long *q_ring;      // list_cap entries: (sequence + 1) << 32 | tile
  uint32_t *q_state, *q_head, *q_tail, *q_pending, *q_done;
  uint32_t *pq_avail, *pq_bits;    // PERSIST == 2: the buckets' counts and bitmaps
  uint32_t pq_bw, pq_shift;
};
__device__ __forceinline__ RelaxQueue relax_queue(uint32_t *tile_list, uint32_t list_cap, uint32_t tiles, uint32_t max_level) {
  RelaxQueue q;
  q.tile_list = tile_list;
  q.list_cap = list_cap;
  q.q_ring = reinterpret_cast<unsigned long long *>(tile_list + RL_HDR);
  q.q_state = tile_list + RL_HDR + 2 * (size_t)list_cap;
  q.q_head = tile_list + RLQ_HEAD; q.q_tail = tile_list + RLQ_TAIL;
  q.q_pending = tile_list + RLQ_PENDING; q.q_done = tile_list + RLQ_DONE;
  q.pq_avail = tile_list + pq_base(list_cap);
  q.pq_bw = pq_words_per_bucket(tiles);
  q.pq_bits = q.pq_avail + PQ_HDR;
  q.pq_shift = pq_shift_of(max_level);
  return q;
}

// List mode, wave 0, all lanes: one "queued for pass p" exchange per candidate (a tile enters a list once: whoever finds the
// old mark adds it), one ticket for the new entries of all of them.
__device__ __forceinline__ void append_flush(uint32_t *tile_list, uint32_t list_cap, uint32_t pass, const uint32_t (&s_cand)[RX_CAND],
                                             uint32_t &s_ncand) {
  const int lane = threadIdx.x & 63;
  const uint32_t n = s_ncand;
  uint32_t *queued = tile_list + RL_HDR + 2 * (size_t)list_cap;
  uint32_t *next = tile_list + RL_HDR + ((pass + 1) & 1u) * (size_t)list_cap;
  const uint32_t mark = pass + 1;
  const bool mine = (uint32_t)lane < n;
  const uint32_t cand = mine ? s_cand[lane] : 0u;
  const bool fresh = mine && atomicExch(&queued[cand], mark) != mark;
  const unsigned long long fm = __builtin_amdgcn_ballot_w64(fresh);
  if (fm) {
    uint32_t at = 0;
    if (lane == 0) at = atomicAdd(&tile_list[(pass + 1) & 3u], (uint32_t)__popcll(fm));
    at = __shfl(at, 0, 64);
    if (fresh) next[at + __popcll(fm & ((1ull << lane) - 1ull))] = cand;
  }
  if (lane == 0) s_ncand = 0;
}

// Take a tile in flood order (PERSIST == 2; the whole workgroup calls, wave 0 works).  Returns the tile + 1, or 0: the queue
// has run dry or the time budget is spent.  q_t0: when this worker began; q_wait / q_polls: its waiting time and looks.
// use_list carries the tuning build's A/B bits (2: quick polls, 4: no back-off).
__device__ __forceinline__ uint32_t queue_take_flood_order(const RelaxQueue &q, unsigned long long q_t0, uint32_t &q_wait, uint32_t &q_polls,
                                                           int use_list, uint32_t &s_qtile, uint32_t &s_qbucket, uint32_t &s_handoff,
                                                           uint32_t (&s_sidemin)[4]) {
  if (threadIdx.x < 64 && s_handoff != 0u) {      // (wave uniform) the run before this one took a tile it had announced itself
    if (threadIdx.x == 0) { s_handoff = 0u; s_sidemin[0] = s_sidemin[1] = s_sidemin[2] = s_sidemin[3] = 0xFFFFFFFFu; }
  } else if (threadIdx.x < 64) {
    const int ln = (int)threadIdx.x;
    const unsigned long long w0 = __builtin_amdgcn_s_memrealtime();
    const uint32_t nchunk = q.pq_bw >> 8;
    uint32_t got = 0, got_b = 0, idle = 0;
    for (;;) {
      // one look at every bucket's count (lane b) and at the end flag (lane 63)
      uint32_t av = 0;
      if (ln < 32) av = __hip_atomic_load(q.pq_avail + ln, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (__shfl((int)av, PQ_B, 64) != 0) break;
      const unsigned long long m = __builtin_amdgcn_ballot_w64(ln < PQ_B && (int)av > 0);
      // (every turn of this loop checks the clock: whatever goes wrong with counts or bits, the end flag is seen a turn later)
      if (ln == 0 && __builtin_amdgcn_s_memrealtime() - q_t0 > RLQ_BUDGET_TICKS) {
        __hip_atomic_store(q.q_done, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(q.pq_avail + PQ_B, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      // A look that ends without a tile -- nothing queued, or somebody else was quicker -- is followed by a pause that grows
      // with the looks in a row: a thousand workers after the same few bits, each look nine memory requests to the same
      // nine lines, held every load of the RUNNING tiles up behind them (a tile run 60 us instead of 15).  Work that
      // appears is found by whoever looks next, so the delay is the pause divided by the number of idle workers.
      auto pause = [&]() {
        ++q_polls;
        ++idle;
        // ... and with the worker's number: sixteen look every 3 us, forty-eight every 14, the rest every 54 -- a front that
        // is a chain of tile runs is followed by the worker that runs it (the hand-off at the end of a run), and a backlog
        // that lasts is found by everybody within one long pause
        const int reps = (use_list & 2) ? 1 : (blockIdx.x < 16u ? 1 : (blockIdx.x < 64u ? 4 : 16));
        if (use_list & 4) __builtin_amdgcn_s_sleep(2);
        else if (idle < 3u) __builtin_amdgcn_s_sleep(8);
        else if (idle < 6u) __builtin_amdgcn_s_sleep(64);
        else { for (int z = 0; z < reps; ++z) __builtin_amdgcn_s_sleep(127); }
      };
      if (m == 0) { pause(); continue; }
      const uint32_t b = (uint32_t)__builtin_ctzll(m);
      uint32_t *bm = q.pq_bits + (size_t)b * q.pq_bw;
      for (uint32_t cc = 0; cc < nchunk; ++cc) {
        const uint32_t c = (cc + blockIdx.x) % nchunk;      // (workers start in different chunks of a long bitmap)
        u32x4_t v;
        coh_load4(v, bm + c * 256u + (uint32_t)ln * 4u);
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(v) : : "memory");
        unsigned long long mm = __builtin_amdgcn_ballot_w64((v.x | v.y | v.z | v.w) != 0u);
        if (mm == 0) continue;
        // workers that look at the same moment take different bits: the k-th lane that has any
        int k = (int)(blockIdx.x % (uint32_t)__popcll(mm));
        while (k-- > 0) mm &= mm - 1ull;
        const int sel = (int)__builtin_ctzll(mm);
        uint32_t t1 = 0, tb = 0;
        if (ln == sel) {
          const int j = v.x ? 0 : (v.y ? 1 : (v.z ? 2 : 3));
          const uint32_t wv = j == 0 ? v.x : (j == 1 ? v.y : (j == 2 ? v.z : v.w));
          const uint32_t bit = wv & (0u - wv);
          const uint32_t wi = c * 256u + (uint32_t)ln * 4u + (uint32_t)j;
          if (atomicAnd(bm + wi, ~bit) & bit) {      // the bit is mine
            atomicSub(q.pq_avail + b, 1u);
            const uint32_t t = (wi << 5) + (uint32_t)__builtin_ctz(bit);
            // not running -> running, every waiting bit taken with it: what they announced was stored before they were set,
            // and this run loads after this exchange.  Running already (a stale bit): that run's end looks at the bits.
            const uint32_t so = atomicMax(&q.q_state[t], PQ_RUNNING);
            if (!(so & PQ_RUNNING)) {
              if (so == 0u) atomicAdd(q.q_pending, 1u);      // (a stale bit of an idle tile: it runs once for nothing)
              t1 = t + 1u;
              tb = so ? (uint32_t)__builtin_ctz(so) : b;
            }
          }
        }
        got = (uint32_t)__shfl((int)t1, sel, 64);
        got_b = (uint32_t)__shfl((int)tb, sel, 64);
        break;      // taken, or somebody else was quicker: look at the counts again
      }
      if (got) break;
      pause();
    }
    if (ln == 0) {
      q_wait += (uint32_t)(__builtin_amdgcn_s_memrealtime() - w0);
      s_qtile = got;
      s_qbucket = got_b;
      s_sidemin[0] = s_sidemin[1] = s_sidemin[2] = s_sidemin[3] = 0xFFFFFFFFu;
    }
  }
  __syncthreads();
  return s_qtile;
}

// Take a tile first come (PERSIST == 1; the whole workgroup calls, thread 0 works): draw a ticket, wait for its entry.
// Returns the tile + 1, or 0: the queue has run dry or the time budget is spent.
__device__ __forceinline__ uint32_t queue_take_first_come(const RelaxQueue &q, unsigned long long q_t0, uint32_t &q_wait, uint32_t &q_polls,
                                                          uint32_t &s_qtile) {
  if (threadIdx.x == 0) {
    unsigned long long v = 0;
    if (__hip_atomic_load(q.q_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) {
      const unsigned long long w0 = __builtin_amdgcn_s_memrealtime();
      const uint32_t my = atomicAdd(q.q_head, 1u);
      unsigned long long *slot = q.q_ring + (my % q.list_cap);
      for (;;) {
        v = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((uint32_t)(v >> 32) == my + 1u) break;      // my entry (not one of the ring's previous lap)
        v = 0;
        ++q_polls;
        if (__hip_atomic_load(q.q_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) break;
        if (__builtin_amdgcn_s_memrealtime() - q_t0 > RLQ_BUDGET_TICKS) { __hip_atomic_store(q.q_done, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
        // Who is next in line polls quickly (the flood is often a chain of tile runs: this wait is on its critical path);
        // who is far behind the tail sleeps longer -- an idle worker must not cost the busy ones their memory bandwidth.
        const uint32_t behind = my - __hip_atomic_load(q.q_tail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // tickets drawn before mine and not yet filled
        if (behind < 4u) __builtin_amdgcn_s_sleep(2);
        else if (behind < 32u) __builtin_amdgcn_s_sleep(24);
        else __builtin_amdgcn_s_sleep(127);
      }
      q_wait += (uint32_t)(__builtin_amdgcn_s_memrealtime() - w0);
      if (v != 0) atomicExch(q.q_state + (uint32_t)v, 2u);      // queued -> running: whoever flags it from now on makes it run again
    }
    s_qtile = v != 0 ? (uint32_t)v + 1u : 0u;
  }
  __syncthreads();
  return s_qtile;
}

// The end of a tile run in flood order (the whole workgroup calls, wave 0 works): hand in the candidates that thread 0 has
// put into s_cand -- tile | bucket << 24 -- and hand the lowest of them off to this worker itself.  self: the tile that ran.
// use_list: the tuning build's A/B bits (8: no hand-off, 16: hand off whatever the bucket).
__device__ __forceinline__ void queue_hand_in_flood_order(const RelaxQueue &q, uint32_t self, int tid, int lane, int use_list,
                                                          const uint32_t (&s_cand)[RX_CAND], uint32_t &s_ncand, uint32_t &s_qtile,
                                                          uint32_t &s_qbucket, uint32_t &s_handoff) {
  __syncthreads();      // thread 0's candidates (s_cand, s_ncand: the append_next block of k_relax) are there
  if (tid < 64) {
    const uint32_t n = s_ncand;
    // my own entry (a run that stopped at its round cap) is lane 63's business: its bit, then "not running any more"
    // in one more exchange that tells me what was announced while I ran
    const bool mine = (uint32_t)lane < n;
    const uint32_t cw = mine ? s_cand[lane] : 0u;
    const uint32_t cand = cw & 0x00FFFFFFu, cb = cw >> 24;      // (relax_pass: the queue is not used on planes of 2^24 tiles)
    const bool other = mine && cand != self;
    // Hand-off: the announced tile of the lowest bucket, if that is no higher than the bucket I ran from (the front I am
    // following), is MY next tile -- one exchange "not running -> running" instead of its bit, its count, some worker's
    // look, claim and exchange: five memory round trips off every hop of a flood that is a chain of tile runs.
    // (Asking the counts instead -- "nothing waits below it", a look issued before the stores -- cost more than it found:
    // one more request per run to the line every worker's counts live on, 4.98 -> 5.32 ms at correlation 64 px.)
    uint32_t pick = other && (cb <= s_qbucket || (use_list & 16)) && !(use_list & 8) ? (cb << 8) | (uint32_t)lane : 0xFFFFu;
#pragma unroll
    for (int k = 1; k < 8; k <<= 1) pick = min(pick, (uint32_t)__shfl_xor((int)pick, k, 64));      // (candidates sit in lanes 0 .. 4)
    pick = (uint32_t)__shfl((int)pick, 0, 64);
    const bool hand = pick != 0xFFFFu && (pick & 0xFFu) == (uint32_t)lane;
    uint32_t old = 0;
    bool taken = false;
    if (hand) {
      old = atomicMax(&q.q_state[cand], PQ_RUNNING);
      taken = !(old & PQ_RUNNING);      // idle (old == 0: mine to count) or queued (its bit goes stale): it is mine now
    }
    if (other && !taken) old = atomicOr(&q.q_state[cand], 1u << cb);
    // idle: mine to queue (and to count); queued in a higher bucket: mine to queue lower, and its old bit goes;
    // queued at or below mine: nothing; running: announced, its run's end queues it
    bool push = other && !taken && !(old & PQ_RUNNING) && (old & ((2u << cb) - 1u)) == 0u;
    const bool fresh = (push || taken) && old == 0u;
    if (taken) { s_handoff = 1u; s_qtile = cand + 1u; s_qbucket = cb; }
    uint32_t pb = cb, pt = cand;
    uint32_t left = 0;
    if (lane == 63) {      // (never a candidate's lane: a run announces five tiles at most)
      const uint32_t c0 = s_cand[0];
      if (n != 0u && (c0 & 0x00FFFFFFu) == self) atomicOr(&q.q_state[self], 1u << (c0 >> 24));
      left = atomicAnd(&q.q_state[self], ~PQ_RUNNING) & ~PQ_RUNNING;
      if (left) { push = true; pb = (uint32_t)__builtin_ctz(left); pt = self; }
    }
    const uint32_t n_fresh = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(fresh));
    if (lane == 63) {
      // counted before anyone can take them; my own run leaves the count in the same add
      const int net = (int)n_fresh - (left ? 0 : 1);
      if (net > 0) atomicAdd(q.q_pending, (uint32_t)net);
      else if (net < 0 && atomicSub(q.q_pending, 1u) == 1u) {
        __hip_atomic_store(q.q_done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(q.pq_avail + PQ_B, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      s_ncand = 0;
#ifdef WS_TUNING
      atomicAdd(q.tile_list + RLQ_RUNS, 1u);
#endif
    }
    if (push) {
      const uint32_t bit = 1u << (pt & 31u);
      if (!(atomicOr(q.pq_bits + (size_t)pb * q.pq_bw + (pt >> 5), bit) & bit)) atomicAdd(q.pq_avail + pb, 1u);
      if (pt != self && old != 0u) {      // lowered: the bit of its former bucket
        const uint32_t ob = (uint32_t)__builtin_ctz(old);
        if (atomicAnd(q.pq_bits + (size_t)ob * q.pq_bw + (pt >> 5), ~bit) & bit) atomicSub(q.pq_avail + ob, 1u);
      }
    }
  }
}

// The end of a tile run first come (the whole workgroup calls, wave 0 works): the candidates in s_cand -- and this tile, if
// somebody flagged it while it ran -- go to the ring's tail.
__device__ __forceinline__ void queue_hand_in_first_come(const RelaxQueue &q, uint32_t self, int tid, int lane, const uint32_t (&s_cand)[RX_CAND],
                                                         uint32_t &s_ncand) {
  __syncthreads();      // thread 0's candidates (s_cand, s_ncand: the append_next block of k_relax) are there
  if (tid < 64) {
    const uint32_t n = s_ncand;
    const bool mine = (uint32_t)lane < n;
    const uint32_t cand = mine ? s_cand[lane] : 0u;
    // idle -> queued: mine to push; queued already: nothing; running: flagged, it queues itself when it ends
    const bool fresh = mine && atomicOr(&q.q_state[cand], 1u) == 0u;
    const unsigned long long fm = __builtin_amdgcn_ballot_w64(fresh);
    const uint32_t nf = (uint32_t)__popcll(fm);
    // my run is over: running -> idle, or -> queued if somebody (I myself, at my round cap) flagged me meanwhile
    uint32_t again = 0;
    if (lane == 0) again = atomicAnd(&q.q_state[self], ~2u) & 1u;
    again = (uint32_t)__shfl((int)again, 0, 64);
    const uint32_t total = nf + again;
    if (total) {
      uint32_t at = 0;
      if (lane == 0) {      // counted before anyone can take them; my own run leaves the count in the same add
        if (total != 1u) atomicAdd(q.q_pending, total - 1u);
        at = atomicAdd(q.q_tail, total);
      }
      at = (uint32_t)__shfl((int)at, 0, 64);
      if (fresh) {
        const uint32_t idx = at + (uint32_t)__popcll(fm & ((1ull << lane) - 1ull));
        __hip_atomic_store(q.q_ring + (idx % q.list_cap), ((unsigned long long)(idx + 1u) << 32) | cand, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      if (lane == 0 && again) {
        const uint32_t idx = at + nf;
        __hip_atomic_store(q.q_ring + (idx % q.list_cap), ((unsigned long long)(idx + 1u) << 32) | self, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    if (lane == 0) {
      s_ncand = 0;
      // nothing queued by me and my run is over: was mine the last tile queued or running?
      if (total == 0u && atomicSub(q.q_pending, 1u) == 1u) __hip_atomic_store(q.q_done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#ifdef WS_TUNING
      atomicAdd(q.tile_list + RLQ_RUNS, 1u);
#endif
    }
  }
}

}  // namespace wsk
