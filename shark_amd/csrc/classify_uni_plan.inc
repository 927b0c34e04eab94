// classify_uni_plan.inc -- a fragment of classify_uni_kernel's BODY (classify_uni.hpp includes it where it stands; not a header of its own):
// geometry of a read (pair) in slots and staging groups; the bound cut's plan (plan_cut) and the sparse first round's (plan_sparse).
  // ---- geometry: of every read of the batch (UNI), of the unit's class (CLS) or of the current read ----------
  const uint32_t k = P.k;
  uint32_t nk1, nk2, P2, g2, n_groups;
  uint32_t tail_inv[G], Lm[G], bofs[G];
  bool act[G], m2[G];
  auto set_geometry = [&](const uint32_t l1, const uint32_t l2) {
    nk1 = l1 >= k ? l1 - k + 1 : 0;
    nk2 = l2 >= k ? l2 - k + 1 : 0;
    P2 = (l1 + 7u) & ~7u;
    g2 = P2 >> 3;
    n_groups = g2 + ((l2 + 7u) >> 3);                 // <= 64 G (UNI: checked before this kernel is chosen; else: per read below)
    // lane -> the 8 bases it stages (per group)
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const uint32_t gi = (uint32_t)lane + 64u * g;
      act[g] = gi < n_groups;
      m2[g] = gi >= g2;
      bofs[g] = (m2[g] ? gi - g2 : gi) << 3;
      Lm[g] = m2[g] ? l2 : l1;
      const uint32_t rem = act[g] ? Lm[g] - bofs[g] : 8u;
      tail_inv[g] = rem < 8u ? (0xFFu << rem) & 0xFFu : 0u;   // positions of the group behind the mate's end
    }
  };
  set_geometry(L1, L2);
  // TRI: 16 bases per lane.  Lane -> (pair of the triple, chunk of the pair); a pair has c1 + c2 chunks, mate 2's first one at packed
  // position P2 = 16 c1.  The 8-base arrays above stay unused but for act[0], which lane_valid_bases() reads: a pair's validity
  // bytes are 2 (c1 + c2).
  uint32_t tri_lp = 0, tri_pr = 0, tri_cl = 0, tri_bofs = 0, tri_tail = 0, tri_Lm = 0;
  bool tri_act = false;
  const uint8_t *tri_base = nullptr;
  // (the tiles' round's results, lanes 0, 1, 2 = pairs 0, 1, 2 of the triple) the lane's pair -- ~0: none, behind every batch's end --
  // and where the pair's sixteen tiles stand in the round's ballot
  const uint32_t tfr_pair = (uint32_t)lane < 3u ? (uint32_t)lane : ~0u;
  const uint32_t tfr_sh = (uint32_t)lane < 3u ? 16u * (uint32_t)lane : 0u;
  if (TRI) {
    const uint32_t c1 = (L1 + 15u) >> 4, c2 = (L2 + 15u) >> 4;
    tri_lp = c1 + c2;
    P2 = c1 << 4;
    g2 = P2 >> 3;
    n_groups = 2u * tri_lp;
    act[0] = (uint32_t)lane < n_groups;
    tri_pr = ((uint32_t)lane >= tri_lp ? 1u : 0u) + ((uint32_t)lane >= 2u * tri_lp ? 1u : 0u);
    tri_cl = (uint32_t)lane - tri_pr * tri_lp;
    tri_act = (uint32_t)lane < 3u * tri_lp;
    const bool in2 = tri_cl >= c1;
    tri_bofs = (in2 ? tri_cl - c1 : tri_cl) << 4;
    tri_Lm = in2 ? L2 : L1;
    const uint32_t rem = tri_act ? tri_Lm - tri_bofs : 16u;       // (>= 1: a chunk holds a base of its mate)
    tri_tail = rem < 16u ? (0xFFFFu << rem) & 0xFFFFu : 0u;
    tri_base = (in2 ? P.seq2 : P.seq1) + tri_bofs;
  }
  // (ragged batches) what a read of the batch brings of its own: slots per mate, and which of a lane's bases lie behind its mate's end
  auto set_read = [&](const uint32_t l1, const uint32_t l2) {
    nk1 = l1 >= k ? l1 - k + 1 : 0;
    nk2 = l2 >= k ? l2 - k + 1 : 0;
#pragma unroll
    for (int g = 0; g < G; ++g) {
      Lm[g] = m2[g] ? l2 : l1;
      const uint32_t rem = Lm[g] > bofs[g] ? Lm[g] - bofs[g] : 0u;
      tail_inv[g] = rem < 8u ? (0xFFu << rem) & 0xFFu : 0u;
    }
  };
  // the bound cut (above): rounds [0, cutE) are probed first; cutUb = bases the slots of the other rounds cover.  cutE = U: no cut
  // ubJA = the same for the stop of the early decision (JA_ROUNDS rounds; vote<J> below)
  constexpr int JA_ROUNDS = (ACCEPT && CutPlan<U>::E0 + 1 < U) ? CutPlan<U>::E0 + 1 : U;
  uint32_t cutE = U, cutUb = 0, ubJA = 0, thr_full = 0;
  auto plan_cut = [&](const uint32_t l1, const uint32_t l2) {
    cutE = U;
    cutUb = 0;
    if (JA_ROUNDS < U) ubJA = bases_behind(64u * (uint32_t)JA_ROUNDS, nk1, nk2, P2, l1, l2);
    thr_full = cov_threshold(P.c, l1 + l2);   // len <= l1 + l2: the joiner is not a valid character
    if (!CUT) return;
    // bases_behind falls with e: the smaller candidate is tried last and wins when it qualifies
    if (CutPlan<U>::E1 != CutPlan<U>::E0) {
      const uint32_t ub = bases_behind(64u * (uint32_t)CutPlan<U>::E1, nk1, nk2, P2, l1, l2);
      if (ub < thr_full) { cutE = (uint32_t)CutPlan<U>::E1; cutUb = ub; }
    }
    const uint32_t ub = bases_behind(64u * (uint32_t)CutPlan<U>::E0, nk1, nk2, P2, l1, l2);
    if (ub < thr_full) { cutE = (uint32_t)CutPlan<U>::E0; cutUb = ub; }
  };
  if (UNI) plan_cut(L1, L2);
  // (three pairs, uniform batch) the thresholds of the batch's pairs, lane i's = that of a pair with i invalid characters: len is
  // L1 + L2 - i, and a pair's count is a popcount of a ballot share when none of its chunks holds two (the tiles' fragment) -- so the
  // double arithmetic of cov_threshold runs once per wave, here, and a pair reads its threshold with one v_readlane.  The same
  // function of the same len: entry by entry what per_pair's reduction gives.  (The offsets form has a pair's own lengths: tro_thr)
  constexpr bool THRTAB = TRI && !TRO;
  uint32_t thr_tab = 0u;
  if constexpr (THRTAB) thr_tab = cov_threshold(P.c, L1 + L2 > (uint32_t)lane ? L1 + L2 - (uint32_t)lane : 0u);
  // (the tiles' round, uniform batch) cnt k >= thr_full as a number of tiles: cnt >= ceil(thr_full / k), once per wave
  uint32_t tf_need = 0u;
  if constexpr (THRTAB) tf_need = k ? (thr_full + k - 1u) / k : 0u;
  // ---- the sparse first round (one-gene index in LDS; DESIGN.md 3).  With ONE gene in the index nothing competes: a read is that
  // gene's iff the bases covered by its k-mers that are in the filter reach c * len, and a LOWER bound on that coverage which
  // passes settles it.  So the 128 probes in front of the cut's stop are made in another order: round A = the even slots of
  // the prefix [0, 128 - T) (57 k-mers that tile 129 bases of mate 1, and an error costs a base or two, not k) plus T tiles --
  // disjoint k-mers k apart, counted back from the last slot of the pair, k bases each --; round B = the rest of the prefix.
  // A read from the gene is through behind round A (2 x 150 bp: 248 of the 180 bases needed, 97 % of the on-target pairs at
  // 1 % errors, instead of behind three rounds and a vote); a read without any match behind B is cut as before, the prefix
  // being what the cut needs (bases_behind(128 - T) < c * len fixes T).  Everything else -- a few per cent -- is brought into the
  // usual order and tried again over the whole prefix and the tiles; what is still open probes the T left-over slots and goes on
  // as ever.  spT = 0: not used (several genes, another geometry).
  // (Ragged batches on a one-gene index run this kernel with the exact table too -- see launch_classify_uni -- and plan per read.)
  constexpr bool SPARSE = LX && CUT && ACCEPT && !SHK_NO_SPARSE && U >= 3 && JA_ROUNDS >= 2 && JA_ROUNDS <= 3;
  uint32_t spT = 0, spLast = 0, spUb = 0;
  // (where a settled read's result goes: held across the loop.  Re-read per read like the vote does, the two dependent scalar
  //  loads were 5 % of an on-target launch: 4.41 -> 4.21 ms per 10 M pairs at 50 % on-target.  Fetching the bases two reads ahead
  //  instead of one was measured as well and changed nothing: 4.21 -> 4.29 ms)
  uint32_t *sp_count = nullptr;
  uint16_t *sp_inl = nullptr;
  // sp_one: ONE gene in the index (the argument above).  Several genes (the LXM instantiation): the same two rounds in the same order
  // settle a read too, by the early decision's argument instead -- see sparse_first
  constexpr bool sp_one = !LXM;
  // SP_STRAIGHT: the pair without a candidate in round A or B -- every pair from elsewhere -- as straight code of its own (per_pair,
  // classify_uni.hpp: the miss path); sparse_first takes over what its two rounds found
  constexpr bool SP_STRAIGHT = SPARSE && sp_one && !SHK_SPARSE_PLAIN;
  // SP_JOINT (a form of SP_STRAIGHT; the k-mer keyed table): the candidate stages of the rounds A and B of a pair as ONE block -- both
  // rounds' windows, both D reads, both T16 reads, then the two ballots.  B's slots are a function of the lane and the plan, not of A's
  // answer, so a pair without a candidate waits for three LDS round trips instead of six; a pair that A alone would have settled has
  // paid B's stage for nothing.  (The hashed forms have no registers for two XXH64 states at once: they keep the serial order.)
  constexpr bool SP_JOINT = SP_STRAIGHT && KX && !SHK_KX_ONE_STAGE && !SHK_SPARSE_SERIAL;
  const bool sp_on = SPARSE && (LXM ? P.lx_multi != 0u : P.lx_gene != 0xFFFFFFFFu);
  // floor(x / k) and floor(x / (k - 1)) for x < 2048 as a multiplication (k <= 32)
  const uint32_t sp_rk = sp_on ? (65536u + k - 1u) / k : 0u, sp_rk1 = (sp_on && k > 1u) ? (65536u + k - 2u) / (k - 1u) : 0u;
  // the smallest slot s with bases_behind(s) <= B
  auto slot_for_ub = [&](const uint32_t B, const uint32_t l1, const uint32_t l2) -> uint32_t {
    const uint32_t c1 = nk1 ? l1 : 0u, c2 = nk2 ? l2 : 0u;   // (a mate shorter than k has no slot and covers nothing)
    if (c1 + c2 <= B) return 0u;
    if (nk1 && c1 + c2 - B < nk1) return c1 + c2 - B;
    if (c2 <= B) return nk1;
    return P2 + (c2 - B < nk2 ? c2 - B : nk2);
  };
  auto plan_sparse = [&](const uint32_t l1, const uint32_t l2) {
    spT = 0;
    if (!sp_on || cutE != 2u || !(nk1 | nk2) || !thr_full) return;
    const uint32_t nkl = nk2 ? nk2 : nk1;
    spLast = (nk2 ? P2 : 0u) + nkl - 1u;                       // the last slot of the pair; tile t is the slot spLast - t k
    // the largest T <= 16 whose tiles stay inside the last mate ((T - 1) k < nkl), do not touch what the prefix covers
    // (spLast - (T - 1) k >= (128 - T) + k - 1, i.e. T (k - 1) <= spLast - 127), and whose prefix still carries the cut
    // (bases_behind(128 - T) < c * len, i.e. 128 - T >= the first slot with at most c * len - 1 bases behind it)
    uint32_t T = 16u;
    const uint32_t t_in = (((nkl - 1u) * sp_rk) >> 16) + 1u;
    T = T < t_in ? T : t_in;
    if (k > 1u) {
      if (spLast < 127u) return;
      const uint32_t t_ap = ((spLast - 127u) * sp_rk1) >> 16;
      T = T < t_ap ? T : t_ap;
    }
    const uint32_t X = slot_for_ub(thr_full - 1u, l1, l2);
    if (X > 127u) return;
    T = T < 128u - X ? T : 128u - X;
    if (T == 0u) return;
    // (the conditions themselves, not their closed forms, decide)
    const uint32_t back = (T - 1u) * k;
    const uint32_t ub = bases_behind(128u - T, nk1, nk2, P2, l1, l2);
    if (back < nkl && spLast >= back && spLast - back >= (128u - T) + k - 1u && ub < thr_full) { spT = T; spUb = ub; }
  };
  if (sp_on) {
    // (through readfirstlane: values of their own from here on.  As plain loads the compiler is free to re-do them at every use when
    //  scalar registers run short -- kernarg -> *P.out -> store, a dependent memory round trip and a vmcnt(0) per settled read; some
    //  builds of the three-pairs kernel did)
    const uint64_t pc = reinterpret_cast<uint64_t>(P.out->count), pi = reinterpret_cast<uint64_t>(P.out->inl);
    sp_count = reinterpret_cast<uint32_t *>(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(pc >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)pc));
    sp_inl = reinterpret_cast<uint16_t *>(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(pi >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)pi));
    if (UNI) plan_sparse(L1, L2);
  }
  // (TRO) the plan of the layout's own lengths, kept: a pair of those lengths takes it as a pair of a uniform batch would
  struct { uint32_t cutE, spT, cutUb, ubJA, thr_full, spLast, spUb; } plan0{cutE, spT, cutUb, ubJA, thr_full, spLast, spUb};
  // (ragged, fixed layout) where the mates' buffers end: off[n]
  uint64_t end1 = 0, end2 = 0;
  if (FIXLAY) {
    end1 = ((ConstU64)(uintptr_t)P.off1)[P.n];
    end2 = P.seq2 ? ((ConstU64)(uintptr_t)P.off2)[P.n] : ~0ull;
  }
  const uint8_t *sbase[G], *qbase[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    sbase[g] = (m2[g] ? P.seq2 : P.seq1) + bofs[g];
    qbase[g] = HASQ ? (m2[g] ? P.qual2 : P.qual1) + bofs[g] : nullptr;
  }
  // the unguarded loads read up to 11 bytes behind a group's first byte: fine while that stays inside the mate's buffer
  // (TRI: the loop below walks TRIPLES of consecutive reads)
  const uint32_t n_reads = (uint32_t)P.n;
  const uint32_t n32 = CLS ? ent_end : (TRI ? (n_reads + 2u) / 3u : n_reads), stride = CLS ? 1u : gridDim.x * WAVES;
  const uint32_t Lmin = L2 ? (L1 < L2 ? L1 : L2) : L1;
  const uint32_t guard_reads = Lmin >= 12u ? 1u : (Lmin ? (12u + Lmin - 1u) / Lmin : n32);   // trailing reads with guarded loads

  // UNI: read r of a mate is at r * L.  The reads a wave fetches are `stride` apart: in the summary / table modes the lane's place in
  // the next one is a running pointer (one 64-bit add per fetch instead of two quarter-rate 64-bit multiply-adds: 1 000 genes at
  // 0 / 50 / 100 % on-target 9.8 / 12.1 / 15.4 -> 9.4 / 11.7 / 15.2 ms per 10 M pairs); the exact-table kernel keeps the product
  // (with the pointer it measured 4.25 -> 4.40 ms)
  constexpr bool RUNPTR = !LX && !DYN;   // (a wave that takes turns has no fixed step)
  const uint8_t *snext[G], *qnext[G];
  uint32_t r_at = blockIdx.x * WAVES + wave;   // the read the running pointers stand at
  {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const uint64_t o = (uint64_t)r_at * Lm[g];
      snext[g] = sbase[g] + o;
      qnext[g] = HASQ ? qbase[g] + o : nullptr;
    }
  }
