// caro_net_kernels.inc -- the three float32 net kernels of caro_net.hip (direct, row Winograd, 2-D Winograd), written
// once and compiled by the includes at the end of namespace cnet's device code -- twice for the depth:
//   CARO_NR = NRES (5), CARO_KN(name) = name        the kernels of the reference's depth: every count a compile-time constant
//   CARO_NR = 0,        CARO_KN(name) = name_any    a tower of any depth 1 .. MAX_NRES: the layer / chunk / tap counts come
//                                                   from the net's own parameter block (p.nres), nothing else differs
// The text is included rather than wrapped in a template: a kernel that forwards its by-value parameter blocks to an
// inlined body does not compile to the instructions of the kernel that owns them.
// and a third time for the FORM of the row-Winograd kernel (the other two kernels exist in the general form only):
//   CARO_SHAPE = ShapeAny,  CARO_ONE_NET = 0    any board, one net or two: shape and tile sizes from the parameter blocks
//   CARO_SHAPE = ShapeC4,   CARO_ONE_NET = 1    k_net_forward_w_c4: connect four's shape as constants, one parameter
//                                               block, which < 2 only (no second net, no struct select)

#if !CARO_ONE_NET
// `which` = 0 / 1: rows of that net only (p0 is used).  `which` = 2: both nets in ONE launch -- tiles
// [0, ceil(L0/TB)) run net 0 on rows [0, L0), the following tiles run net 1 (p1) on rows [L0, L0+L1).
__global__ __launch_bounds__(NT, 2) void CARO_KN(k_net_forward)(NetParams p0, NetParams p1, const float* __restrict__ planes,
                                                         const int32_t* __restrict__ counts, int which, int row1,
                                                         float* __restrict__ probs, float* __restrict__ values,
                                                         unsigned long long* __restrict__ stamps,
                                                         const int32_t* __restrict__ gpack, int gG, int gB) {
  __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
  float* act = lds;
  float* wbuf = lds + ACT;

  int L, row0, board0;
  bool second = false;
  if (which < 2) {
    L = counts[which];
    row0 = which ? counts[0] : 0;
    board0 = blockIdx.x * p0.TB;
  } else {
    const int L0 = counts[0];
    const int t0 = (L0 + p0.TB - 1) / p0.TB;
    second = (int)blockIdx.x >= t0;
    L = second ? counts[1] : L0;
    row0 = second ? (row1 >= 0 ? row1 : L0) : 0;
    board0 = (second ? (int)blockIdx.x - t0 : (int)blockIdx.x) * p0.TB;
  }
  if (board0 >= L) return;
  const NetParams p = second ? p1 : p0;
  const float slope = p.slope;
  // diagnostic only (stamps == nullptr in every product launch): shader clock vs 100 MHz wall clock
  unsigned long long t_c0 = 0, t_r0 = 0;
  if (stamps) {
    t_c0 = __builtin_amdgcn_s_memtime();
    t_r0 = __builtin_amdgcn_s_memrealtime();
  }
  const int nb = min(p.TB, L - board0);
  const int HW = p.HW;
  const int R = nb * HW;  // real rows
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int i = lane & 31, h = lane >> 5;

  // zero the activation buffer (dummy rows and the zero row stay zero for ever)
  for (int k = tid; k < ACT / 4; k += NT) reinterpret_cast<float4*>(lds)[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  // conv_in weights into wbuf: [9][2][64] = 1152 floats
  for (int k = tid; k < 9 * 2 * NF; k += NT) wbuf[k] = p.w_in[k];
  int* smap = reinterpret_cast<int*>(wbuf + 1536);  // [TB] plane / output row of every board of this tile
  tile_rows(gpack, gG, gB, second ? 1 : 0, row0 + board0, board0, nb, smap + 64, smap, tid);  // ends with a barrier

  conv_in_f32(p, planes, smap, act, wbuf, R, tid);
  const int slot_v = tid < nb ? smap[tid] : 0;
  __syncthreads();

  unsigned long long t_trunk0 = 0;
  if (stamps) t_trunk0 = __builtin_amdgcn_s_memtime();
  // ---- stage weight chunk 0 (taps 0 and 1 of layer 0)
  {
    const float4* src = reinterpret_cast<const float4*>(p.w_res);
#pragma unroll
    for (int m = 0; m < 2 * TPC; ++m) reinterpret_cast<float4*>(wbuf)[tid + NT * m] = src[tid + NT * m];
  }
  __syncthreads();

  // per-lane geometry of its row tile
  const int myrow = wave * 32 + i;
  const bool rvalid = myrow < R;
  const int rbi = myrow / HW;
  const int rcell = myrow - rbi * HW;
  const int ry = rcell / p.W, rx = rcell - ry * p.W;
  const int bswz = (i >> 1) & 7;

  f32x16 acc0, acc1;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    acc0[e] = 0.f;
    acc1[e] = 0.f;
  }
  static_assert(TPC == 3, "the staging registers below are written out for three taps per chunk");
  float4 wn0, wn1, wn2, wn3, wn4, wn5;  // next weight chunk in flight (lives across the taps of a chunk)
  wn0 = wn1 = wn2 = wn3 = wn4 = wn5 = make_float4(0.f, 0.f, 0.f, 0.f);
  const int ntaps = (CARO_NR ? CARO_NR : p.nres) * 9, nchunk = (ntaps + TPC - 1) / TPC;
  for (int ft = 0; ft < ntaps; ++ft) {  // flat tap index over the residual layers
    const int c = ft / TPC, within = ft % TPC, cur = c & 1;
    const int layer = ft / 9, tap = ft % 9;
    const bool last_in_chunk = within == TPC - 1 || ft == ntaps - 1;
    const bool has_next = c + 1 < nchunk;
    if (within == 0 && has_next) {  // issue early
      const float4* src = reinterpret_cast<const float4*>(p.w_res + (size_t)(c + 1) * TPC * WCHUNK);
      wn0 = src[tid];
      wn1 = src[tid + NT];
      wn2 = src[tid + 2 * NT];
      wn3 = src[tid + 3 * NT];
      wn4 = src[tid + 4 * NT];
      wn5 = src[tid + 5 * NT];
    }
    const float* wcur = wbuf + cur * TPC * WCHUNK + within * WCHUNK;
    const int ny = ry + tap / 3 - 1, nx = rx + tap % 3 - 1;
    const bool ok = rvalid && ny >= 0 && ny < p.H && nx >= 0 && nx < p.W;
    const int nrow = ok ? rbi * HW + ny * p.W + nx : ZROW;
    const float* abase = act + nrow * NF;
    const int aswz = nrow & 15;
    const float* bbase0 = wcur + (h * 64 + i) * 32;
    const float* bbase1 = wcur + (h * 64 + 32 + i) * 32;
    // software pipeline with two explicit operand register sets: the reads of group q+1 are ISSUED before the
    // eight MFMAs of group q (sched_barrier keeps hipcc from sinking them next to their consumers, which it
    // otherwise does to save registers and which exposes one LDS latency per group)
#define CARO_LOAD_SET(A_, B0_, B1_, Q_)                                                             \
  A_ = *reinterpret_cast<const float4*>(abase + (((h * 8 + (Q_)) ^ aswz) << 2));                    \
  B0_ = *reinterpret_cast<const float4*>(bbase0 + (((Q_) ^ bswz) << 2));                            \
  B1_ = *reinterpret_cast<const float4*>(bbase1 + (((Q_) ^ bswz) << 2));
#define CARO_MFMA_SET(A_, B0_, B1_)                                                \
  acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(A_.x, B0_.x, acc0, 0, 0, 0);        \
  acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(A_.x, B1_.x, acc1, 0, 0, 0);        \
  acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(A_.y, B0_.y, acc0, 0, 0, 0);        \
  acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(A_.y, B1_.y, acc1, 0, 0, 0);        \
  acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(A_.z, B0_.z, acc0, 0, 0, 0);        \
  acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(A_.z, B1_.z, acc1, 0, 0, 0);        \
  acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(A_.w, B0_.w, acc0, 0, 0, 0);        \
  acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(A_.w, B1_.w, acc1, 0, 0, 0);
    float4 xa, xb0, xb1, ya, yb0, yb1;
    CARO_LOAD_SET(xa, xb0, xb1, 0)
#pragma unroll
    for (int q = 0; q < 8; q += 2) {
      CARO_LOAD_SET(ya, yb0, yb1, q + 1)
      __builtin_amdgcn_sched_barrier(0);
      CARO_MFMA_SET(xa, xb0, xb1)
      __builtin_amdgcn_sched_barrier(0);
      if (q + 2 < 8) {
        CARO_LOAD_SET(xa, xb0, xb1, q + 2)
      }
      __builtin_amdgcn_sched_barrier(0);
      CARO_MFMA_SET(ya, yb0, yb1)
      __builtin_amdgcn_sched_barrier(0);
    }
#undef CARO_LOAD_SET
#undef CARO_MFMA_SET
    if (last_in_chunk && has_next) {  // write late: the other buffer was last read one chunk ago
      float4* dst = reinterpret_cast<float4*>(wbuf + (cur ^ 1) * TPC * WCHUNK);
      dst[tid] = wn0;
      dst[tid + NT] = wn1;
      dst[tid + 2 * NT] = wn2;
      dst[tid + 3 * NT] = wn3;
      dst[tid + 4 * NT] = wn4;
      dst[tid + 5 * NT] = wn5;
    }
    if (tap == 8) {
      __syncthreads();  // every wave has read this layer's input activations: they may be overwritten
      // epilogue, in place: v = v + leaky(conv(v) + b)   (lib/model.py:85-89).  Branch-free: rows >= R (dummy
      // rows and the zero row) are rewritten with zeros; all 32 residual reads are issued before the first use.
      const float* bias = p.b_res + layer * NF;
      const float bc0 = bias[i], bc1 = bias[32 + i];
      float old0[16], old1[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        old0[e] = act[aoff(row, i)];
        old1[e] = act[aoff(row, 32 + i)];
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        const bool real = row < R;
        const float n0 = old0[e] + leaky(acc0[e] + bc0, slope);
        const float n1 = old1[e] + leaky(acc1[e] + bc1, slope);
        act[aoff(row, i)] = real ? n0 : 0.f;
        act[aoff(row, 32 + i)] = real ? n1 : 0.f;
        acc0[e] = 0.f;
        acc1[e] = 0.f;
      }
    }
    if (last_in_chunk || tap == 8) __syncthreads();  // staged weights / new activations visible to every wave
  }
  unsigned long long t_trunk1 = 0;
  if (stamps) t_trunk1 = __builtin_amdgcn_s_memtime();
  // `act` now holds the trunk output; the weight stage is free scratch
  heads_f32<ShapeAny, false>(p, act, wbuf, probs, values, slot_v, nb, R, tid);
  if (stamps && tid == 0) {
    stamps[4 * blockIdx.x] = __builtin_amdgcn_s_memtime() - t_c0;
    stamps[4 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime() - t_r0;
    stamps[4 * blockIdx.x + 2] = t_trunk0 - t_c0;
    stamps[4 * blockIdx.x + 3] = t_trunk1 - t_c0;
  }
}
#endif  // !CARO_ONE_NET

#if CARO_ONE_NET
__global__ __launch_bounds__(NT, 2) void CARO_KN(k_net_forward_w)(NetParams p0, const float* __restrict__ planes,
                                                           const int32_t* __restrict__ counts, int which,
                                                           float* __restrict__ probs, float* __restrict__ values,
                                                           unsigned long long* __restrict__ stamps,
                                                           const int32_t* __restrict__ gpack, int gG, int gB) {
#else
__global__ __launch_bounds__(NT, 2) void CARO_KN(k_net_forward_w)(NetParams p0, NetParams p1,
                                                           const float* __restrict__ planes,
                                                           const int32_t* __restrict__ counts, int which, int row1,
                                                           float* __restrict__ probs, float* __restrict__ values,
                                                           unsigned long long* __restrict__ stamps,
                                                           const int32_t* __restrict__ gpack, int gG, int gB) {
#endif
  using S = CARO_SHAPE;  // every board quantity below comes from its accessors
  __shared__ __attribute__((aligned(256))) float lds[LDS_FLOATS];  // trunk_w XORs granule bits into LDS addresses
  float* act = lds;
  float* wbuf = lds + ACT;

  /*@PST(0)*/
  const unsigned long long t_abs0 = stamps ? __builtin_amdgcn_s_memrealtime() : 0;  // diagnostic only
  // slot form: this thread's share of the games' leaf counts is requested beside the launch's totals (tile_rows_pre)
  const int gcpt = gpack ? (gG + NT - 1) / NT : 0;
  const bool gpre = gpack && gcpt <= GP_PRE;
  int gv[GP_PRE];
#pragma unroll
  for (int u = 0; u < GP_PRE; ++u) {
    const int g = (int)threadIdx.x * gcpt + u;
    gv[u] = gpre && u < gcpt && g < gG ? gpack[g] : 0;
  }
  const int TB = S::TB(p0.TB), TB2 = S::TB2(p0.TB2), TB4 = S::TB4(p0.TB4);
  int L, row0, board0, nb, nb_cap = TB;
  int ks = 1;  // K-split of this workgroup's tiles (1: a full tile of TB boards)
#if CARO_ONE_NET
  constexpr bool second = false;
  {
#else
  bool second = false;
  if (which < 2) {
#endif
    L = counts[which];
    row0 = which ? counts[0] : 0;
    board0 = blockIdx.x * TB;
    // Tile size by launch size.  A full tile is TB boards (128 GEMM rows); smaller tiles split the K loop over the
    // waves instead (2-way: TB2 boards, 0.6 of a full tile's time; 4-way: TB4 boards, 0.4).  One round of the chip
    // holds ncu workgroups, so
    //   L <= ncu * TB4 / ncu * TB2 : every tile is a 4-way / 2-way tile (small launches finish sooner);
    //   L a little above one round of full tiles: workgroups [0, ncu) stay full, the overflow goes into small
    //   tiles and the second round is short;
    //   otherwise full tiles.
    const int full = p0.ncu * TB;
    if (p0.ncu > 0) {
      if (TB4 > 0 && L <= p0.ncu * TB4) ks = 4;
      else if (TB2 > 0 && L <= p0.ncu * TB2) ks = 2;
      if (ks > 1) {
        nb_cap = ks == 4 ? TB4 : TB2;
        board0 = (int)blockIdx.x * nb_cap;
      } else if (L > full) {
        const int over = L - full;
        if (TB4 > 0 && over <= p0.ncu * TB4) ks = 4;
        else if (TB2 > 0 && over <= p0.ncu * TB2) ks = 2;
        if (ks > 1) {
          if ((int)blockIdx.x < p0.ncu) {
            ks = 1;
          } else {
            nb_cap = ks == 4 ? TB4 : TB2;
            board0 = full + ((int)blockIdx.x - p0.ncu) * nb_cap;
          }
        }
      }
    }
  }
#if !CARO_ONE_NET
  else {
    // two nets in one launch: the tile size follows the sum (one workgroup of slack: each class rounds up)
    const int L0 = counts[0], L1 = counts[1];
    if (p0.ncu > 1) {
      if (TB4 > 0 && L0 + L1 <= (p0.ncu - 1) * TB4) ks = 4;
      else if (TB2 > 0 && L0 + L1 <= (p0.ncu - 1) * TB2) ks = 2;
      if (ks > 1) nb_cap = ks == 4 ? TB4 : TB2;
    }
    const int t0 = (L0 + nb_cap - 1) / nb_cap;
    second = (int)blockIdx.x >= t0;
    L = second ? L1 : L0;
    row0 = second ? (row1 >= 0 ? row1 : L0) : 0;
    board0 = (second ? (int)blockIdx.x - t0 : (int)blockIdx.x) * nb_cap;
  }
#endif
  if (board0 >= L) return;
  /*@PST(1)*/
#if CARO_ONE_NET
  const NetParams& p = p0;
#else
  const NetParams p = second ? p1 : p0;
#endif
  unsigned long long t_c0 = 0, t_r0 = 0;  // diagnostic only, as in k_net_forward
  if (stamps) {
    t_c0 = __builtin_amdgcn_s_memtime();
    t_r0 = __builtin_amdgcn_s_memrealtime();
  }
  nb = min(nb_cap, L - board0);
  const int HW = S::HW(p.HW);
  const int R = nb * HW;  // real rows
  const int tid = threadIdx.x;

  // this thread's leaf count of the tile's class: consumed HERE, in front of the weight transfers (the wait for gv is
  // then a wait for gv alone)
  int gmine = 0;
#pragma unroll
  for (int u = 0; u < GP_PRE; ++u) gmine += (gv[u] >> 8) == (second ? 1 : 0) ? (gv[u] & 0xFF) : 0;
  asm volatile("" : "+v"(gmine));
  // the first two weight chunks are on their way into ring buffers 0 and 1 while conv_in runs; its scratch (the
  // conv_in weights, the row map) sits in buffer 2, which is fetched into only after the trunk's first barrier
  float* win = wbuf + 2 * WCH;
  // conv_in's weights first (1152 floats: the first five waves move 16 bytes per lane, b_in and a few floats more
  // come along), then the two chunks: the wait below is for the oldest transfer only
  if (tid < 320) dma_b128(reinterpret_cast<const float4*>(p.w_in) + tid,
                          __builtin_amdgcn_readfirstlane(lds_addr(win) + (unsigned)(tid >> 6) * 1024u));
  fetch_chunk(p.ww, 0, lds_addr(wbuf), tid);
  fetch_chunk(p.ww, 1, lds_addr(wbuf), tid);
  // rows of boards this tile does not have, the spare rows and the zero row stay zero for ever; the others are written
  // by conv_in
  for (int k = tid + (R * NF) / 4; k < ACT / 4; k += NT) reinterpret_cast<float4*>(lds)[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  // the wait below leaves exactly this thread's 2 chunks x (WCH / 4 / NT) transfers in flight (conv_in's weights are
  // the oldest transfer): the immediate is tied to the constants here.  conv_in reads w_in from LDS and b_in from
  // global memory, so only w_in has to be covered by the 320-lane transfer (what comes along behind it is not used).
  static_assert(2 * (WCH / 4 / NT) == 8, "s_waitcnt vmcnt(8) below counts 2 chunks x WCH / 4 / NT transfers per thread");
  static_assert(320 * 4 >= 9 * 2 * NF, "the 320-lane transfer must cover w_in [9][2][64]");
  /*@PST(2)*/
  asm volatile("s_waitcnt vmcnt(8)" ::: "memory");  // the 2 x 4 chunk transfers of this thread may still be on their way
  /*@PST(3)*/
  int* smap = reinterpret_cast<int*>(win + 1536);  // [TB] plane / output row of every board of this tile
  if (gpre) tile_rows_pre(gv, gcpt, gmine, gB, second ? 1 : 0, board0, nb, smap + 64, smap, tid);  // ends with a barrier
  else tile_rows(gpack, gG, gB, second ? 1 : 0, row0 + board0, board0, nb, smap + 64, smap, tid);
  /*@PST(4)*/
  conv_in_mfma<S>(p, planes, smap, act, win, R, tid);
  /*@PST(5)*/
  const int slot_v = tid < nb ? smap[tid] : 0;
  unsigned long long t_trunk0 = 0;
  if (stamps) t_trunk0 = __builtin_amdgcn_s_memtime();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();  // conv_in's output and the two chunks are visible to every wave
  /*@PST(6)*/
  // head parameters staged in LDS during the trunk's last chunks when they fit (heads_f32)
  // (a fixed shape is one whose block fits, ShapeFixed: hspan is a constant and the unstaged heads are not instantiated)
  const int hspan = head_span(HW, S::A(p.A)) <= HEAD_STAGE_MAX ? head_span(HW, S::A(p.A)) : 0;
  if (ks == 1) trunk_w<1, CARO_NR, S>(p, act, wbuf, nb, tid, hspan);
  else if (ks == 2) trunk_w<2, CARO_NR, S>(p, act, wbuf, nb, tid, hspan);
  else trunk_w<4, CARO_NR, S>(p, act, wbuf, nb, tid, hspan);
  unsigned long long t_trunk1 = 0;
  if (stamps) t_trunk1 = __builtin_amdgcn_s_memtime();
  /*@PST(8)*/
#if CARO_ONE_NET
  static_assert(S::FIXED, "the one-net form is built for a fixed shape, whose head block is always staged");
  heads_f32<S, true>(p, act, wbuf, probs, values, slot_v, nb, R, tid);
#else
  if (hspan) heads_f32<S, true>(p, act, wbuf, probs, values, slot_v, nb, R, tid);
  else heads_f32<S, false>(p, act, wbuf, probs, values, slot_v, nb, R, tid);
#endif
  /*@PST(12)*/
  if (stamps && tid == 0) {
    stamps[4 * blockIdx.x] = __builtin_amdgcn_s_memtime() - t_c0;
    // slot launches (the engine's own: caro_net_debug_stamps) carry the wall clock of the workgroup's START above bit 20
    stamps[4 * blockIdx.x + 1] = gpack ? ((__builtin_amdgcn_s_memrealtime() - t_abs0) & 0xFFFFFull) | (t_abs0 << 20)
                                       : __builtin_amdgcn_s_memrealtime() - t_r0;
    stamps[4 * blockIdx.x + 2] = t_trunk0 - t_c0;
    stamps[4 * blockIdx.x + 3] = t_trunk1 - t_c0;
    /*@HST_PUBLISH(stamps, wbuf)*/
  }
}

#if !CARO_ONE_NET
// One board per workgroup (TB = 1); launch interface, prologue (slot-row map, conv_in on the matrix pipe) and heads of
// k_net_forward_w, activation rows keyed by akey<true>.
__global__ __launch_bounds__(NT, 2) void CARO_KN(k_net_forward_w2)(NetParams p0, NetParams p1,
                                                            const float* __restrict__ planes,
                                                            const int32_t* __restrict__ counts, int which, int row1,
                                                            float* __restrict__ probs, float* __restrict__ values,
                                                            unsigned long long* __restrict__ stamps,
                                                            const int32_t* __restrict__ gpack, int gG, int gB,
                                                            float* __restrict__ featbuf, int32_t* __restrict__ rowlist,
                                                            const int32_t* __restrict__ slist) {
  __shared__ __attribute__((aligned(256))) float lds[LDS_FLOATS];  // trunk_w2d XORs granule bits into LDS addresses
  float* act = lds;
  float* wbuf = lds + ACT;
  // slot form: this thread's share of the games' leaf counts is requested beside the launch's totals (tile_rows_pre).
  // slist (caro_net_forward_slot_list): the slot row of every dense board comes from the producer's list instead -- one
  // board per workgroup leaves no tile to fill, so no workgroup needs the prefix sum over the G leaf counts (1.2 us of
  // each workgroup: 37 us of a 7 600-board launch), and which dense index a board got does not touch its arithmetic
  const int gcpt = gpack && !slist ? (gG + NT - 1) / NT : 0;
  const bool gpre = gpack && !slist && gcpt <= GP_PRE;
  int gv[GP_PRE];
#pragma unroll
  for (int u = 0; u < GP_PRE; ++u) {
    const int g = (int)threadIdx.x * gcpt + u;
    gv[u] = gpre && u < gcpt && g < gG ? gpack[g] : 0;
  }
  int L, row0, board0;
  bool second = false;
  if (which < 2) {
    L = counts[which];
    row0 = which ? counts[0] : 0;
    board0 = blockIdx.x;
  } else {
    const int L0 = counts[0];
    second = (int)blockIdx.x >= L0;
    L = second ? counts[1] : L0;
    row0 = second ? (row1 >= 0 ? row1 : L0) : 0;
    board0 = second ? (int)blockIdx.x - L0 : (int)blockIdx.x;
  }
  if (board0 >= L) return;
  const int listed = slist ? slist[(second ? gG * gB : 0) + board0] : 0;  // (requested here, used behind conv_in's weights)
  const NetParams p = second ? p1 : p0;
  unsigned long long t_c0 = 0, t_r0 = 0;  // diagnostic only (stamps == nullptr in every product launch)
  if (stamps) {
    t_c0 = __builtin_amdgcn_s_memtime();
    t_r0 = __builtin_amdgcn_s_memrealtime();
  }
  const int nb = 1;
  const int HW = p.HW;
  const int R = HW;
  const int tid = threadIdx.x;
  int gmine = 0;
#pragma unroll
  for (int u = 0; u < GP_PRE; ++u) gmine += (gv[u] >> 8) == (second ? 1 : 0) ? (gv[u] & 0xFF) : 0;
  asm volatile("" : "+v"(gmine));
  // the first two weight chunks are on their way into ring buffers 0 and 1 while conv_in runs; its scratch (the conv_in
  // weights, the row map) sits in buffer 2, which is fetched into only after the trunk's first barrier
  float* win = wbuf + 2 * WCH;
  if (tid < 320) dma_b128(reinterpret_cast<const float4*>(p.w_in) + tid,
                          __builtin_amdgcn_readfirstlane(lds_addr(win) + (unsigned)(tid >> 6) * 1024u));
  fetch_chunk_s(p.ww2, 0, lds_addr(wbuf), tid);
  fetch_chunk_s(p.ww2, 1, lds_addr(wbuf), tid);
  for (int k = tid + (R * NF) / 4; k < ACT / 4; k += NT) reinterpret_cast<float4*>(lds)[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  static_assert(2 * (WCH / 4 / NT) == 8, "s_waitcnt vmcnt(8) below counts 2 chunks x WCH / 4 / NT transfers per thread");
  asm volatile("s_waitcnt vmcnt(8)" ::: "memory");  // conv_in's weights have arrived; the 2 x 4 chunk transfers may be on their way
  int* smap = reinterpret_cast<int*>(win + 1536);
  if (slist) {
    if (tid == 0) smap[0] = listed;
    __syncthreads();
  } else if (gpre) tile_rows_pre(gv, gcpt, gmine, gB, second ? 1 : 0, board0, nb, smap + 64, smap, tid);  // ends with a barrier
  else tile_rows(gpack, gG, gB, second ? 1 : 0, row0 + board0, board0, nb, smap + 64, smap, tid);
  conv_in_mfma<ShapeAny, true>(p, planes, smap, act, win, R, tid);
  const int slot_v = tid < nb ? smap[tid] : 0;
  unsigned long long t_trunk0 = 0;
  if (stamps) t_trunk0 = __builtin_amdgcn_s_memtime();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();  // conv_in's output and the two chunks are visible to every wave
  trunk_w2d<CARO_NR>(p, act, wbuf, tid);
  unsigned long long t_trunk1 = 0;
  if (stamps) t_trunk1 = __builtin_amdgcn_s_memtime();
  // featbuf != null: the FC heads of the whole launch follow in k_net_heads (row0 + board0 = this board's dense index)
  heads_f32<ShapeAny, false, true>(p, act, wbuf, probs, values, slot_v, nb, R, tid, featbuf, rowlist, row0 + board0);
  if (stamps && tid == 0) {
    stamps[4 * blockIdx.x] = __builtin_amdgcn_s_memtime() - t_c0;
    stamps[4 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime() - t_r0;
    stamps[4 * blockIdx.x + 2] = t_trunk0 - t_c0;
    stamps[4 * blockIdx.x + 3] = t_trunk1 - t_c0;
  }
}
#endif  // !CARO_ONE_NET
