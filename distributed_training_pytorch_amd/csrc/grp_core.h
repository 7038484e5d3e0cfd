// On-chip all-reduce among the GR workgroups that share ONE model's batch inside one
// launch (the split-batch step of mlp_train_lanes.hip: a model's per-rank batch spread over GR
// CUs, each running the several-lanes step on batch / GR samples; and the members of a
// layer-split stage, split_lanes.hip).
//
// Why: the one-lane step at batch 256 keeps one CU per model busy and is latency-bound
// (4.1 us/step); the 4-lanes step does 64 samples in ~2.2 us.  Splitting the batch over
// GR = batch / 64 workgroups and summing their partial weight gradients on chip before
// the (redundant, bitwise identical) optimizer step trades ~half the step's chain for
// one on-chip hand-off.
//
// Protocol: the granule form of xgmi_core.h at device scope (MI355X_MICROARCH.md
// "Workgroup dispatch ... inter-workgroup visibility", recipe R2 of
// cdna_hip_programming.md Guideline 16):
//   * one coarse-grained device buffer, layout [parity 2][model][src workgroup][slot] of
//     16-byte granules {epoch ^ h(v), v0, v1, v2}: three payload floats, and a tag word that
//     carries the check -- a granule passes only as tag ^ h(v) == epoch, so a stale slot of
//     an earlier epoch never passes and a torn one only on a hash collision.  A member's
//     payload is its P gradients, its loss and its XCC id: grp_ng3(P) granules;
//   * a workgroup stores each of its granules ONCE (every member reads the same slot --
//     no per-peer copies as over xGMI), with ONE 16-byte write-through (sc1) store;
//   * members poll the other GR - 1 slots with sc1 loads (L1 bypassed, so no acquire
//     fence is needed: every load of the handed-off bytes is an sc1 load and every store
//     an sc1 store) until the tag matches; the own contribution stays on chip;
//   * the roles are split over the waves: wave 0 publishes the member's granules, waves 1..
//     poll the peers'.  On gfx9 loads and stores share ONE in-order vmcnt, so a wave that
//     polls right after its own publish stores cannot consume its first poll before those
//     write-through stores are acknowledged (measured: one poll after the publish took
//     ~2.9 k cycles, every peer granule already there).  Pollers that never stored see a
//     plain load round trip.  The pollers start after a barrier behind the publisher's store
//     issue, so the stores enter the CU's memory pipeline ahead of sweeps of lines that
//     cannot be there yet.  The peers' values meet the member's own in LDS;
//   * sums run in workgroup order 0..GR-1 on every member -> bitwise identical gradients,
//     hence bitwise identical optimizer steps and weight replicas in every member;
//   * two parities + a monotonic epoch (device counter, never rewound): a member can run
//     at most one exchange ahead of another, so exchange e+1 never overwrites a slot still
//     being read for exchange e, and a granule from an earlier launch never matches;
//   * spins are bounded; a timeout sets status[0] / status[1] = epoch, the step continues
//     (what an earlier exchange left in the LDS rows stands in for the missing items: the
//     status word already marks the run failed, check_comm raises, whatever the values).
// Placement: the members of a model are blocks m, m + 8, m + 16, ... (one XCD under the
// observed round-robin dispatch, so the hand-off stays in that XCD's L2) -- speed only:
// the protocol is correct under any placement (sc1 on both sides).  After a launch's first
// exchange (write-through stores) has shown every member of the model on ONE XCD, the
// members publish with plain stores: the lines stay in that XCD's L2 and the sc1 polls hit
// there (a write-through store drops its line from L2, so a poll of it reads beyond L2).
// Each member sends its XCC id with its payload, so every member takes the same decision;
// members on different XCDs keep write-through.
// The experiments this form came out of are in docs/perf_notes.md ("Retired compile-time
// switches").
#pragma once
#include "xgmi_core.h"

namespace dtp {

constexpr int kGrpMax = 8;  // workgroups per model (batch <= 512 at 64 samples each)

constexpr int kGrpStAux = 16;  // granule stores: sc1 (write-through, device scope)
constexpr int kGrpLdAux = 16;  // granule polls: sc1 (L2-served, L1 bypassed)

// granules per (parity, model, member) slot -- the xGMI slot size (xgmi_core.h)
DTP_HD constexpr int grp_slot16(int P, int npt) { return xgmi_slot16(P, npt); }

// 3-float granules of a member: the P gradients, the loss and the member's XCC id (125 for
// the toy shape: 2 poll items per lane at 4 members)
DTP_HD constexpr int grp_ng3(int P) { return (P + 2 + 2) / 3; }
// LDS floats per member (pub, then one row per member)
DTP_HD constexpr int grp_ps3(int P) { return (3 * grp_ng3(P) + 3) & ~3; }
DTP_DEV uint32_t grp_hash3(uint32_t a, uint32_t b, uint32_t c) {
  return a ^ ((b << 11) | (b >> 21)) ^ ((c << 22) | (c >> 10)) ^ 0x9E3779B9u;
}

// The split-batch members park their per-wave dW tiles in PAYLOAD order: one row per wave,
// payload float f (parameter f, the loss at P) at grp_row_pos(f).  A row's granule q is
// floats [4q, 4q + 3), one pad float (aligned 16-byte reads).
DTP_HD constexpr int grp_row_pos(int f) { return 4 * (f / 3) + f % 3; }
DTP_HD constexpr int grp_row_floats(int P) { return 4 * grp_ng3(P); }

struct GrpCtx {
  void* buf;    // [2][n_models][GR][slot16] granules
  int* status;  // sticky timeout word pair (nullable)
  int GR, k, n_models, timeout_us;
};

// diagnostic (PROF instances only): s_memtime when the publish stores were issued, when the
// first poll was consumed and when the last granule arrived, and the number of polls
struct GrpProf {
  unsigned long long t_pub, t_first, t_end;
  unsigned polls;
  unsigned long long rt_pub = 0, rt_end = 0;  // s_memrealtime (chip-wide 100 MHz): publisher done, last granule
};

DTP_DEV unsigned grp_xcc_id() {
  unsigned x;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
  return x & 0xFu;
}

DTP_DEV unsigned long long grp_clock() {
  unsigned long long t;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}

// The exchange.  g (in): this member's partial sums of its NPT owned parameters (thread t
// owns parameters NPT t ..); out: the sums over the GR members.  Returns the summed loss.
// Called by every thread of the member.
//   lds: (1 + kGrpMax) rows of grp_ps3(P) floats -- pub, then peer[r]: member r's payload
//   dead: the caller's sticky timeout flag (read from the status word once per launch; a
//     poller that times out tells its workgroup through the status word, every thread of
//     the member takes the flag from there at the next launch)
//   xcc: this member's XCC id; plain (in/out, per launch, starts false): publish with plain
//     stores, set once every member is known to share this XCD
//   GRC > 0: the member count as a constant (the caller guarantees c.GR == GRC): the poll
//     items per lane and the sums' trip counts are constants
// Staged form (RNW = 0): the owners stage the member's payload in pub (gradients p = 0..P-1,
// the loss at P, the XCC id at P + 1), one barrier, wave 0 publishes granule q = floats
// [3q, 3q + 3), waves 1.. poll the peers' granules into their rows, one poll in flight (the
// lane's item count is the one for this member count; every poll requests all of them).
// Row form (RNW > 0): the member's per-wave partial sums are parked in RNW payload-order
// rows (rows + w * RSTRIDE, grp_row_pos).  Wave 0 forms granule q from one float4 per row,
// summed in wave order from 0.f -- the operations of the caller's own() sums, so it publishes
// the bits the member adds for itself -- with no staging pass and no staging barrier; pub
// is not used.  own() fills g and loss from the rows (LDS reads only, counted on lgkmcnt, not
// on the polls' vmcnt): the pollers run it between their first poll's issue and its
// consumption, wave 0 behind the publisher-first barrier.  Every read of the rows completes
// before the final barrier, so the next step's park never races with them.
template <int P, int NPT, int NTHREADS, int GRC = 0, int RNW = 0, int RSTRIDE = 0, class OwnFn = std::nullptr_t>
DTP_DEV float grp_allreduce3(const GrpCtx& c, int model, float (&g)[NPT], const float& loss, unsigned epoch, int tid,
                             bool& dead, float* __restrict__ lds, unsigned xcc, bool& plain, GrpProf* prof,
                             const float* __restrict__ rows = nullptr, OwnFn own = nullptr) {
  constexpr int NG = grp_ng3(P), PS = grp_ps3(P);
  constexpr bool kRows = RNW > 0;
  static_assert(!kRows || (!std::is_same_v<OwnFn, std::nullptr_t> && RSTRIDE % 4 == 0 && RSTRIDE >= 4 * NG),
                "the row form needs the caller's own sums and 16-byte aligned rows of NG granules");
  const int GR = GRC > 0 ? GRC : c.GR;
  constexpr int NPOLL = NTHREADS - kWave;  // poller lanes (waves 1..)
  constexpr int slot = grp_slot16(P, NPT);
  static_assert(NG <= slot, "a member's 3-float granules fit its slot of the exchange buffer");
  static_assert(NTHREADS > kWave, "one publisher wave and at least one poller wave");
  float* const pub = lds;
  float* const peer = lds + PS;  // peer[r * PS + i]: member r's float i
  // the addresses are those of parity 0 (per-launch values once inlined in the step loop);
  // the parity's half of the buffer is the scalar offset operand of the loads and stores
  const int par = __builtin_amdgcn_readfirstlane((int)(epoch & 1u));
  const int soff = par ? c.n_models * GR * slot * 16 : 0;
  auto goff = [&](int r, int q) { return ((model * GR + r) * slot + q) * 16; };  // byte offset of granule q of member r
  // 1. the payload into LDS
  if constexpr (!kRows) {
#pragma unroll
    for (int k = 0; k < NPT; ++k)
      if (NPT * tid + k < P) pub[NPT * tid + k] = g[k];
    if (tid == 0) {
      pub[P] = loss;
      pub[P + 1] = __uint_as_float(xcc);
#pragma unroll
      for (int i = P + 2; i < 3 * NG; ++i) pub[i] = 0.f;
    }
    __syncthreads();
  }
  const __amdgpu_buffer_rsrc_t rs = xgmi_rsrc(c.buf);
  if (tid < kWave) {
    // 2a. wave 0 publishes every granule of this member (all its LDS reads first, then the
    // stores back to back)
    constexpr int MAXJ = (NG + kWave - 1) / kWave;
    float v[MAXJ][3];
    if constexpr (kRows) {
      float4 t[MAXJ][RNW];
#pragma unroll
      for (int j = 0; j < MAXJ; ++j) {
        const int q = tid + j * kWave < NG ? tid + j * kWave : NG - 1;
#pragma unroll
        for (int w = 0; w < RNW; ++w) t[j][w] = *reinterpret_cast<const float4*>(rows + w * RSTRIDE + 4 * q);
      }
#pragma unroll
      for (int j = 0; j < MAXJ; ++j) {
        const int q = tid + j * kWave < NG ? tid + j * kWave : NG - 1;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int w = 0; w < RNW; ++w) {
          s0 += t[j][w].x;
          s1 += t[j][w].y;
          s2 += t[j][w].z;
        }
        // past the loss: the XCC id at float P + 1, then zeros (the rows hold nothing there)
        const float xf = __uint_as_float(xcc);
        v[j][0] = 3 * q == P + 1 ? xf : (3 * q > P + 1 ? 0.f : s0);
        v[j][1] = 3 * q + 1 == P + 1 ? xf : (3 * q + 1 > P + 1 ? 0.f : s1);
        v[j][2] = 3 * q + 2 == P + 1 ? xf : (3 * q + 2 > P + 1 ? 0.f : s2);
      }
    } else {
#pragma unroll
      for (int j = 0; j < MAXJ; ++j) {
        const int q = tid + j * kWave < NG ? tid + j * kWave : NG - 1;
        v[j][0] = pub[3 * q];
        v[j][1] = pub[3 * q + 1];
        v[j][2] = pub[3 * q + 2];
      }
    }
    // plain is the same on every lane of wave 0 (decided from the same LDS words; the
    // publisher never polls, so never times out): as a scalar, the store's aux choice is one
    // scalar branch
    const bool pst = __builtin_amdgcn_readfirstlane((int)plain) != 0;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
      const int q = tid + j * kWave;
      if (q < NG) {
        const uint32_t x0 = __float_as_uint(v[j][0]), x1 = __float_as_uint(v[j][1]), x2 = __float_as_uint(v[j][2]);
        const u32x4 qq = {epoch ^ grp_hash3(x0, x1, x2), x0, x1, x2};
        const int off = goff(c.k, q);
        if (pst) __builtin_amdgcn_raw_buffer_store_b128(qq, rs, off, soff, 0);
        else __builtin_amdgcn_raw_buffer_store_b128(qq, rs, off, soff, kGrpStAux);
      }
    }
    if (prof) {
      prof->t_pub = grp_clock();
      prof->rt_pub = __builtin_amdgcn_s_memrealtime();
    }
  }
  __syncthreads();  // the pollers start behind the publisher's store issue
  if constexpr (kRows) {
    if (tid < kWave) own();  // behind the barrier: the pollers do not wait for these sums
  }
  if (tid >= kWave) {
    // 2b. item i = (peer index i / NG, granule i % NG), lane pl holds items pl + j NPOLL
    const int pl = tid - kWave;
    const int total = (GR - 1) * NG;
    unsigned long long deadline = 0;
    unsigned spins = 0;
    if (prof) prof->t_pub = grp_clock();
    // the clock is an SMEM read (it would hold the next LDS wait at lgkmcnt(0)): read it only
    // every 64 polls
    auto expired = [&]() {
      if ((++spins & 63u) != 0u) return false;
      const unsigned long long now = __builtin_amdgcn_s_memrealtime();
      if (!deadline) {
        deadline = now + (unsigned long long)(c.timeout_us > 0 ? c.timeout_us : 2000000) * 100ull;
      } else if (now > deadline) {
        if (c.status) {
          atomicExch(&c.status[0], 1);
          atomicExch(&c.status[1], (int)epoch);
        }
        return true;
      }
      return false;
    };
    // PI items per lane, one poll in flight; every poll requests all PI items (a fixed load
    // count keeps the waits counted), absent items read offset 0
    auto run = [&](auto PIC) {
      constexpr int PI = decltype(PIC)::value;
      int off[PI], dst[PI];
      uint32_t pending = 0u;
#pragma unroll
      for (int j = 0; j < PI; ++j) {
        const int i = pl + j * NPOLL;
        const int ri = i / NG, q = i - ri * NG;
        const int r = ri < c.k ? ri : ri + 1;
        const bool in = i < total;
        off[j] = in ? goff(r, q) : 0;
        dst[j] = r * PS + 3 * q;
        if (in) pending |= 1u << j;
      }
      auto issue = [&](u32x4 (&x)[PI]) {
        asm volatile("" ::: "memory");  // a poll is never merged with, or hoisted above, an earlier one
#pragma unroll
        for (int j = 0; j < PI; ++j) x[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, off[j], soff, kGrpLdAux);
      };
      auto consume = [&](const u32x4 (&x)[PI]) {
#pragma unroll
        for (int j = 0; j < PI; ++j) {
          if (((pending >> j) & 1u) && (x[j].x ^ grp_hash3(x[j].y, x[j].z, x[j].w)) == epoch) {
            float* d = peer + dst[j];
            d[0] = __uint_as_float(x[j].y);
            d[1] = __uint_as_float(x[j].z);
            d[2] = __uint_as_float(x[j].w);
            pending &= ~(1u << j);
          }
        }
      };
      u32x4 xa[PI];
      if constexpr (kRows) {
        // the first poll goes out, the own sums run while it is in flight (exactly once, also
        // on a lane without items and in a dead launch)
        if (pending && !dead) issue(xa);
        own();
        while (pending && !dead) {
          consume(xa);
          if (prof && spins == 0) prof->t_first = grp_clock();
          if (!pending) break;
          if (expired()) {
            dead = true;
            break;
          }
          issue(xa);
        }
      } else {
        while (pending && !dead) {
          issue(xa);
          consume(xa);
          if (prof && spins == 0) prof->t_first = grp_clock();
          if (pending && expired()) dead = true;
        }
      }
    };
    constexpr int MAXI = ((kGrpMax - 1) * NG + NPOLL - 1) / NPOLL;
    if constexpr (GRC > 0) {  // the member count is a constant: so is the lane's item count
      constexpr int pic = ((GRC - 1) * NG + NPOLL - 1) / NPOLL;
      run(std::integral_constant<int, (pic <= 1 ? 1 : pic <= 3 ? pic : MAXI)>{});
    } else {
      const int pi = (total + NPOLL - 1) / NPOLL;
      if (pi <= 1) run(std::integral_constant<int, 1>{});
      else if (pi <= 2) run(std::integral_constant<int, 2>{});
      else if (pi <= 3) run(std::integral_constant<int, 3>{});
      else run(std::integral_constant<int, MAXI>{});
    }
    if (prof) {
      prof->t_end = grp_clock();
      prof->polls = spins + 1;
      prof->rt_end = __builtin_amdgcn_s_memrealtime();
    }
  }
  __syncthreads();
  // 3. member-order sums
  if (!plain && !dead) {  // every member on this XCD: plain stores from the next exchange on
    bool same = true;
    for (int r = 0; r < GR; ++r)
      if (r != c.k) same = same && __float_as_uint(peer[r * PS + P + 1]) == xcc;
    plain = same;
  }
  float acc[NPT], lacc = 0.f;
#pragma unroll
  for (int k = 0; k < NPT; ++k) acc[k] = 0.f;
  const int p0 = NPT * tid < P ? NPT * tid : 0;
  // Without a branch per member: every thread puts its own sums into its own member's row --
  // no poller writes row c.k, and a thread reads back only what it wrote itself (the LDS
  // queue is in order); a slot it does not own goes to the row's XCC float, which nobody
  // reads in the own row -- then all GR rows are read alike (aligned 8-byte reads for 2
  // parameters), in member order.
  // Some of these reads return values nobody defined, and every one of them is discarded:
  // the own row's loss float row[P] is never written (rl gives way to loss in the select
  // below; the last owner of an odd P also gets it as its second float, a slot it does not
  // own), and a thread past the owners (p0 = 0) reads floats 0 and 1 of the own row while
  // thread 0 writes them.  The sums of unowned slots end in the optimizer's unowned
  // registers, whose weights go to the sink.  The unowned stores all hit float P + 1.
  float* const mine = peer + c.k * PS;
#pragma unroll
  for (int k = 0; k < NPT; ++k) mine[NPT * tid + k < P ? NPT * tid + k : P + 1] = g[k];
  for (int r = 0; r < GR; ++r) {
    const float* row = peer + r * PS;
    if constexpr (NPT == 2 && PS % 2 == 0) {
      const float2 t = *reinterpret_cast<const float2*>(row + p0);
      acc[0] += t.x;
      acc[1] += t.y;
    } else {
#pragma unroll
      for (int k = 0; k < NPT; ++k) acc[k] += row[p0 + k];
    }
    const float rl = row[P];
    lacc += r == c.k ? loss : rl;
  }
#pragma unroll
  for (int k = 0; k < NPT; ++k) g[k] = acc[k];
  return lacc;
}

// the staged form: g and loss are the caller's sums
template <int P, int NPT, int NTHREADS>
DTP_DEV float grp_allreduce_split3(const GrpCtx& c, int model, float (&g)[NPT], float loss, unsigned epoch, int tid,
                                   bool& dead, float* __restrict__ lds, unsigned xcc, bool& plain, GrpProf* prof) {
  return grp_allreduce3<P, NPT, NTHREADS>(c, model, g, loss, epoch, tid, dead, lds, xcc, plain, prof);
}

// the row form: published from RNW payload-order rows, own() forms g and loss from them
// inside the exchange
template <int P, int NPT, int NTHREADS, int GRC, int RNW, int RSTRIDE, class OwnFn>
DTP_DEV float grp_allreduce_rows3(const GrpCtx& c, int model, float (&g)[NPT], const float& loss, unsigned epoch,
                                  int tid, bool& dead, float* __restrict__ lds, unsigned xcc, bool& plain,
                                  GrpProf* prof, const float* __restrict__ rows, OwnFn own) {
  return grp_allreduce3<P, NPT, NTHREADS, GRC, RNW, RSTRIDE>(c, model, g, loss, epoch, tid, dead, lds, xcc, plain,
                                                             prof, rows, own);
}

}  // namespace dtp
