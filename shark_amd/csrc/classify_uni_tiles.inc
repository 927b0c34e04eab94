// classify_uni_tiles.inc -- a fragment of classify_uni_kernel's BODY (classify_uni.hpp includes it where it stands; not a header of its own):
// a probe of the exact LDS table (lx_probe), which pairs of a triple hold invalid characters, and the tiles' round in front of three staged pairs (TF).
    // the slot ss of a staged pair (its two code streams at fwp / rvp) as a probe of the exact LDS table (LX): is its k-mer in the
    // filter?  payload = the gene of the matched entry's single-gene list, or the escape value.  (Not validated: the caller looks
    // at the slot when something matched.)
    // `sparse` (a constant; KX): the probe is one of a round in which a miss is the expected answer -- what comes back is then the
    // CANDIDATE stage's answer (kmer_table.hpp) with `tag` and `s2` for the confirm stage, which the caller runs behind the ballot it
    // takes over the round's hits anyway (lx_confirm); otherwise tag and s2 are not touched and the answer is final
    auto lx_probe = [&](const uint32_t *fwp, const uint32_t *rvp, const uint32_t ss, uint32_t &payload, auto sparse, uint32_t &tag, uint32_t &s2) -> bool {
      const uint32_t q = rcap - k - ss;
      const uint32_t *f = fwp + (ss >> 4);
      const uint32_t *r = rvp + (q >> 4);
      const uint32_t d0 = f[0], d1 = f[1], d2 = f[2];
      const uint32_t e0 = r[0], e1 = r[1], e2 = r[2];
      const uint32_t af = (ss & 15u) << 1, ar = (q & 15u) << 1;
      const uint64_t x = ((uint64_t)__builtin_amdgcn_alignbit(d2, d1, af) << 32) | __builtin_amdgcn_alignbit(d1, d0, af);
      const uint64_t y = ((uint64_t)__builtin_amdgcn_alignbit(e2, e1, ar) << 32) | __builtin_amdgcn_alignbit(e1, e0, ar);
      const uint64_t fwd = y & kmer_mask, rc = ~x & kmer_mask;
      if constexpr (KX) {
        // the table keyed by the canonical k-mer itself (kmer_table.hpp): no XXH64; every entry is the one gene's (P.lx_gene), none escapes.
        // Where misses are expected every lane compares the tag's low 16 bits only; the entry's other two bits and the two guards are
        // looked at when some lane of the wave passed that -- one probe stream in a thousand among reads from elsewhere, and every
        // hit's.  The tiles' round, where nearly every probe is a hit, asks the whole rule at once
        payload = 0u;
        const uint8_t *img = reinterpret_cast<const uint8_t *>(lsum);
        if constexpr (decltype(sparse)::value && !SHK_KX_ONE_STAGE) return kxtab_candidate(img, P.lsum_shift, P.kx_m2, fwd < rc ? fwd : rc, tag, s2);
        else return kxtab_lookup(img, P.lsum_shift, P.kx_m2, fwd < rc ? fwd : rc);
      }
      const uint64_t h = xxh64_u64(fwd < rc ? fwd : rc);
      const uint32_t *T = lsum;
      const char *D = reinterpret_cast<const char *>(lsum + LTAB_T_WORDS);
      const uint32_t tagmask15 = (uint32_t)(P.bf_mask >> LTAB_SLOT_LG);
      const uint32_t gmask2 = (tagmask15 & ((1u << LTAB_GROUP_LG) - 1u)) << 1;
      const uint32_t dd = *reinterpret_cast<const uint16_t *>(D + (((uint32_t)h >> (LTAB_SLOT_LG - 1)) & gmask2));
      const uint32_t tg = __builtin_amdgcn_alignbit((uint32_t)(h >> 32), (uint32_t)h, LTAB_SLOT_LG) & tagmask15;
      const uint32_t base = (uint32_t)h + (tg >> LTAB_GROUP_LG) * P.lsum_shift;
      const uint32_t ee = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(T) + (((base + dd) << 2) & ((LTAB_T_WORDS - 1u) << 2)));
      payload = ee & LTAB_ESC;
      return (ee >> 13) == ((tg << 1) | 1u);
    };
    // (SP_JOINT) the candidate stages of TWO slots of a staged pair -- a lane's slot of round A and its slot of round B -- stage by
    // stage: the twelve window dwords, the two mixes, the two D reads, the two T16 reads.  Each answer is kxtab_candidate's for its
    // slot (the same reads, the same compare); written out here so that no read of B's stands behind a wait for A's
    auto lx_candidates2 = [&](const uint32_t *fwp, const uint32_t *rvp, const uint32_t sa, const uint32_t sb, bool &ha, uint32_t &tga, uint32_t &s2a,
                              bool &hb, uint32_t &tgb, uint32_t &s2b) {
      if constexpr (KX) {
        const uint32_t qa = rcap - k - sa, qb = rcap - k - sb;
        const uint32_t *fa = fwp + (sa >> 4), *ra = rvp + (qa >> 4), *fb = fwp + (sb >> 4), *rb = rvp + (qb >> 4);
        const uint32_t a0 = fa[0], a1 = fa[1], a2 = fa[2], c0 = ra[0], c1 = ra[1], c2 = ra[2];
        const uint32_t b0 = fb[0], b1 = fb[1], b2 = fb[2], e0 = rb[0], e1 = rb[1], e2 = rb[2];
        auto canon = [&](const uint32_t d0, const uint32_t d1, const uint32_t d2, const uint32_t r0, const uint32_t r1, const uint32_t r2, const uint32_t ss, const uint32_t q) -> uint64_t {
          const uint32_t af = (ss & 15u) << 1, ar = (q & 15u) << 1;
          const uint64_t x = ((uint64_t)__builtin_amdgcn_alignbit(d2, d1, af) << 32) | __builtin_amdgcn_alignbit(d1, d0, af);
          const uint64_t y = ((uint64_t)__builtin_amdgcn_alignbit(r2, r1, ar) << 32) | __builtin_amdgcn_alignbit(r1, r0, ar);
          const uint64_t fwd = y & kmer_mask, rc = ~x & kmer_mask;
          return fwd < rc ? fwd : rc;
        };
        const uint8_t *img = reinterpret_cast<const uint8_t *>(lsum);
        uint32_t basea, baseb;
        kxtab_mix(canon(a0, a1, a2, c0, c1, c2, sa, qa), P.lsum_shift, P.kx_m2, tga, basea);
        kxtab_mix(canon(b0, b1, b2, e0, e1, e2, sb, qb), P.lsum_shift, P.kx_m2, tgb, baseb);
        const uint32_t da = *reinterpret_cast<const uint16_t *>(img + KXTAB_D_OFF + ((tga << 1) & ((2u << KXTAB_GROUP_LG) - 2u)));
        const uint32_t db = *reinterpret_cast<const uint16_t *>(img + KXTAB_D_OFF + ((tgb << 1) & ((2u << KXTAB_GROUP_LG) - 2u)));
        s2a = ((basea + da) << 1) & ((2u << KXTAB_RING_LG) - 2u);
        s2b = ((baseb + db) << 1) & ((2u << KXTAB_RING_LG) - 2u);
        const uint16_t ta = *reinterpret_cast<const uint16_t *>(img + s2a);
        const uint16_t tb = *reinterpret_cast<const uint16_t *>(img + s2b);
        ha = ta == (uint16_t)tga;
        hb = tb == (uint16_t)tgb;
      }
    };
    // the confirm stage of a sparse-round candidate (true where lx_probe's answer was final already)
    auto lx_confirm = [&](const uint32_t tag, const uint32_t s2) -> bool {
      if constexpr (KX && !SHK_KX_ONE_STAGE) return kxtab_confirm(reinterpret_cast<const uint8_t *>(lsum), tag, s2);
      else return true;
    };
    // (TRI) does pair p of the triple hold an invalid character (N)?  -- its threshold is then lower than the plan's, and its slots need
    // their validity windows: per_pair's business
    // (uniform batch, THRTAB) two ballots per triple instead of one per pair: the chunks with an invalid character, and the chunks with
    // more than one.  Pair p's share of either is tri_lp bits from bit p tri_lp (a lane outside the triple has inv_real = 0).  The first
    // share says whether the pair holds one at all; where the second share is empty its popcount IS the number of the pair's invalid
    // characters (one per chunk, at most 21) -- all but a few pairs in a thousand at an N per 500 bases -- and thr_tab has the threshold
    bool inv3[3] = {false, false, false};
    uint64_t inv_any = 0ull, inv_two = 0ull;
    if constexpr (THRTAB) {
      inv_any = __ballot(inv_real != 0u);
      inv_two = __ballot((inv_real & (inv_real - 1u)) != 0u);
#pragma unroll
      for (uint32_t p3 = 0; p3 < 3u; ++p3) inv3[p3] = ((inv_any >> (p3 * tri_lp)) & ((1ull << tri_lp) - 1ull)) != 0ull;
    } else if (TRI) {
#pragma unroll
      for (uint32_t p3 = 0; p3 < 3u; ++p3) inv3[p3] = __ballot((inv_real != 0u) & (tri_pr == p3)) != 0ull;
    }
    // TF: the tiles' round (see above) -- bit p of tf_done: pair p of the triple is settled
    uint32_t tf_done = 0u;
    if constexpr (TF) {
      if (tf_on) {
        uint32_t pay, tg_ = 0u, s2_ = 0u;
        const uint32_t *fwp = reinterpret_cast<const uint32_t *>(wbase + tf_area * WORDS);
        bool hit = tf_want & lx_probe(fwp, fwp + code_dwords_for(S), tf_slot, pay, std::false_type{}, tg_, s2_);
        if (inv3[0] | inv3[1] | inv3[2] | (TRO && tro_short != 0u)) {   // (TRO: a tile behind a short mate's end is no k-mer of the pair; the staging marked those bases invalid)
          // a pair with invalid characters: a tile counts when its k characters are valid (slot_valid's window); the pair's threshold
          // is at most the plan's (fewer valid bases), so the plan's is the safe one to pass
          const uint64_t *vb = reinterpret_cast<const uint64_t *>(fwp) + code_dwords_for(S);   // (the area's validity words behind its two code streams)
          const uint32_t V = tf_slot >> 6, vs = tf_slot & 63u;
          const uint64_t v0 = vb[V], v1 = vb[V + 1];
          const uint64_t win = (v0 >> vs) | ((v1 << 1) << (63u - vs)), km = (1ull << k) - 1ull;
          hit = hit & ((win & km) == km);
        }
        const uint64_t Hb = __ballot(hit);
        // (the hashed offsets form stands at 128 VGPRs with XXH64's state and spills with one lane constant more: it keeps the form below)
        constexpr bool TF_BY_LANES = !SHK_TRI_PLAIN && !(TRO && !KX);
        // lanes 0, 1, 2 each own pair p = lane: its sixteen tiles' popcount and its threshold per lane, ONE ballot for the three verdicts
        // -- tf_done is that ballot, a scalar by construction --, and under it one store of the three counts (consecutive dwords) and
        // one of the three inline entries (24 consecutive bytes), from a scalar base and the lane's constant offset
        // (TRO: tro_thr holds pair p's own threshold in lane p -- of its two lengths; a pair with N has a lower one still: passing this
        //  one is sufficient.  Uniform batch: tf_need tiles, the plan's threshold as a number of tiles)
        if constexpr (TF_BY_LANES) {
          // (the asm statements are empty: they keep a scalar a scalar -- left to itself the compiler adds the lane's number to 3 it, and
          //  to both addresses, with a v_mad_u64_u32 each)
          uint32_t it3 = 3u * it;
          asm("" : "+s"(it3));
          // (the offsets form stands at 128 VGPRs: it keeps ONE lane constant and shifts it here, three full-rate instructions a triple;
          //  the shift by 16 (~0): bits 48 ... of the ballot, and the lane has no pair)
          uint32_t tfr_p = tfr_pair, tfr_s = tfr_sh;
          if constexpr (TRO) {
            asm volatile("" : "+v"(tfr_p));
            tfr_s = tfr_p << 4;
          }
          const uint32_t cnt = (uint32_t)__builtin_popcount((uint32_t)(Hb >> (tfr_s & 63u)) & 0xFFFFu);
          bool pass = tfr_p < n_reads - it3;               // (it3 < n_reads; a lane behind the third has no pair: tfr_pair = ~0)
          if constexpr (TRO && !(SHK_TRO_ABL & 2)) pass = pass && tro_thr != 0u && __umul24(cnt, k) >= tro_thr;
          else if constexpr (TRO) pass = pass && thr_full != 0u && __umul24(cnt, k) >= thr_full;
          else pass = pass && cnt >= tf_need;
          tf_done = (uint32_t)__builtin_amdgcn_ballot_w64(pass);
          if (pass && !SHK_ABL(P, 64u)) {
            // (global, not flat: the scalar base stays in its two SGPRs, the lane's offset is the instruction's vector operand)
            typedef __attribute__((address_space(1))) uint32_t GlobalU32;
            typedef __attribute__((address_space(1))) uint64_t GlobalU64;
            typedef __attribute__((address_space(1))) char GlobalChar;
            constexpr uint32_t INL_BYTES = (uint32_t)(SHK_INLINE_IDS * sizeof(uint16_t));
            GlobalChar *cb = (GlobalChar *)sp_count + 4ull * it3;
            GlobalChar *ib = (GlobalChar *)sp_inl + (uint64_t)INL_BYTES * it3;
            uint32_t co = tfr_p << 2, io = tfr_p * INL_BYTES;
            asm("" : "+s"(cb), "+s"(ib), "+v"(co), "+v"(io));   // (the offsets too: widened to 64 bits in front of the loop they are no operand of the store any more)
            *(GlobalU32 *)(cb + co) = 1u;
            *(GlobalU64 *)(ib + io) = (uint64_t)(P.lx_gene & 0xFFFFu);   // {the gene, 0, 0, 0}
          }
        } else {
#pragma unroll
        for (uint32_t p3 = 0; p3 < 3u; ++p3) {
          const uint32_t cnt = (uint32_t)__builtin_popcount((uint32_t)(Hb >> (16u * p3)) & 0xFFFFu);
          const uint32_t rd = 3u * it + p3;
          // (said to be uniform in so many words: taken for a per-lane value, tf_done lived in a vector register and every pair of the
          //  triple behind an exec-mask branch)
          // (TRO: the pair's own threshold -- of its two lengths; a pair with N has a lower one still: passing this one is sufficient)
          const uint32_t thr_p = (TRO && !(SHK_TRO_ABL & 2)) ? (uint32_t)__builtin_amdgcn_readlane((int)tro_thr, (int)p3) : thr_full;      // (TRO: thr_full is the last pair's)
          if (__builtin_amdgcn_readfirstlane((int)((!TRO || thr_p != 0u) && cnt * k >= thr_p && rd < n_reads))) {
            if (lane == 0 && !SHK_ABL(P, 64u)) {
              sp_count[rd] = 1u;
              uint2 pk;
              pk.x = P.lx_gene & 0xFFFFu;
              pk.y = 0u;
              *reinterpret_cast<uint2 *>(sp_inl + (uint64_t)rd * SHK_INLINE_IDS) = pk;
            }
            tf_done |= 1u << p3;
          }
        }
        }
      }
    }
