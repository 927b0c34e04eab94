// classify_uni_sparse.inc -- a fragment of classify_uni_kernel's BODY (classify_uni.hpp includes it where it stands; not a header of its own):
// the bound cut at a stop (ruled_out), a slot as a probe of the LDS table with validation (lx_hit_at), the sparse first round(s) of indices held in LDS (sparse_first).
    // the bound cut at a stop behind the rounds [0, J): what is in the filter so far covers `cv` bases, the slots not probed
    // yet cover `ub`: together fewer than c * len -- no gene can reach the threshold (ReadAnalyzer.hpp:104), the read has no
    // association.  LDS modes stop only without any match (their matches are not validated yet, and a gene's k-mers are rare
    // among an off-target read's); the table modes -- large references, where a random k-mer IS in the filter every few dozen
    // slots -- count what the matches cover: the union of everything found first, then the largest coverage for ONE gene.
    auto ruled_out = [&](auto j_const, const uint32_t ub, const bool per_gene) -> bool {
      if (ub >= thr_r) return false;
      if (!__ballot(lane_any)) return true;
      if (!TOL) return false;
      if (found_cover(j_const) < thr_r - ub) return true;
      return per_gene && gene_cover(j_const) < thr_r - ub;
    };
    // the slot ss of the read as a probe of the exact LDS table (LX): is its k-mer in the filter?  (`want` false: no probe)
    // (KX: the candidate stage's answer; the caller confirms behind its ballot with lx_confirm(tag, s2) -- the sparse rounds' reads
    //  are nearly all from elsewhere behind the tiles' round)
    auto lx_hit_at = [&](const uint32_t ss_in, const bool want, uint32_t &payload, uint32_t &tag, uint32_t &s2) -> bool {
      return want & lx_probe(fw, rv, want ? ss_in : 0u, payload, std::true_type{}, tag, s2);
    };
    // the first two rounds of a one-gene index in the sparse order (see spT above).  true: the read is settled.  false: mt / slo of
    // the rounds 0 and 1 are what probe_rounds would have left (matches validated), the read goes on behind the cut's first stop.
    // Returns 1: the read is settled.  0: not settled, mt / slo of the rounds 0 and 1 are what probe_rounds would have left (one-gene
    // indices).  2: not settled and nothing left behind -- the caller probes the first rounds in the usual order (indices of several
    // genes: a read whose matches are not all one gene's single-gene lists, or do not reach the threshold yet; rare).
    // SEVERAL GENES.  Every entry of the exact table carries its list's one gene (or the escape value: a list of several genes, a
    // gene beyond 13 bits).  Say every match of the rounds A and B -- the whole prefix [0, 128 - T) and the T tiles -- is a
    // single-gene list of ONE gene g, and what those matches cover (as the vote counts it) is cov.  Any other gene's k-mers can
    // then only sit in slots that were not probed, all at packed positions >= 128 - T, which cover at most spUb bases: its final
    // coverage is <= spUb, while g's is >= cov.  With cov >= c * len (thr_r) and cov > spUb, g is the read's only association
    // (ReadAnalyzer.hpp:90-108) whatever the other 140 probes would say: 128 probes instead of 192 and no vote -- the early
    // decision's argument (above), made one round earlier because the tiles bring mate 2's coverage forward.
    auto sparse_first = [&]() -> int {
      const uint32_t T = spT, nA = 64u - T, ln = (uint32_t)lane;
      // (the read's one association)
      auto write_the_gene = [&](const uint32_t g) {
        if (lane == 0 && !SHK_ABL(P, 64u)) {
          sp_count[read] = 1u;
          uint2 pk;
          pk.x = g & 0xFFFFu;
          pk.y = 0u;
          *reinterpret_cast<uint2 *>(sp_inl + (uint64_t)read * SHK_INLINE_IDS) = pk;
        }
      };
      const bool tile = ln >= nA;
      const uint32_t sA = tile ? spLast - (ln - nA) * k : 2u * ln;
      const uint32_t sB = ln < nA - 1u ? 2u * ln + 1u : ln + nA;
      uint32_t pA = 0u, pB = 0u, tgA = 0u, tgB = 0u, s2A = 0u, s2B = 0u;
      bool hA, hB = false;
      uint64_t HA, HB = 0ull;
      if constexpr (SP_STRAIGHT) {
        // round A's candidate stage was per_pair's (the miss path, classify_uni.hpp) -- and round B's too where A had no candidate
        // (SP_JOINT: always, beside A's): what they left is taken over, no round is probed twice
        // (the empty asm: A's ballot is looked at again here, two scalar instructions -- told where it came from, the compiler carries
        //  "B was probed" as a lane mask of its own from there to here, spilled on the way)
        hA = mp_hA; HA = mp_HA; tgA = mp_tgA; s2A = mp_s2A;
        asm volatile("" : "+s"(HA));
      } else {
        SHK_STAMP(2);
        hA = lx_hit_at(sA, true, pA, tgA, s2A);
        HA = __ballot(hA);
        SHK_STAMP(3);
      }
      if (SP_STRAIGHT && !SP_JOINT && !HA) {
        hB = mp_hB; HB = mp_HB; tgB = mp_tgB; s2B = mp_s2B;
      } else {
        if (HA) {
          hA = hA && lx_confirm(tgA, s2A) && slot_valid(sA);   // (the entry's other bits; the slot has to exist and be a valid k-mer)
          HA = __ballot(hA);
        }
        if (HA && sp_one) {
          // bases covered by what matched: an even slot adds min(k, distance to the next even match), a tile k
          const uint64_t H1 = HA & ((1ull << nA) - 1ull);
          const uint64_t nx = (H1 >> ln) >> 1;
          const uint32_t step = nx ? 2u * ((uint32_t)__builtin_ctzll(nx) + 1u) : k;
          const uint32_t cov = wave_sum_u32((hA && !tile) ? (step < k ? step : k) : 0u) + k * (uint32_t)__builtin_popcountll(HA >> nA);
          if (cov >= thr_r) {
            write_the_gene(P.lx_gene);
            SHK_STAMP(4);
            return 1;
          }
        }
        SHK_STAMP(4);
        if constexpr (SP_JOINT) {
          // (B's candidate stage ran beside A's in per_pair, whatever A's answer: taken over here, behind A's coverage)
          hB = mp_hB; HB = mp_HB; tgB = mp_tgB; s2B = mp_s2B;
        } else {
          hB = lx_hit_at(sB, true, pB, tgB, s2B);
          HB = __ballot(hB);
          SHK_STAMP(5);
        }
      }
      // (a pair with a candidate in A or B joins here, hA / tgA / s2A and B's as the rounds left them: no round is probed twice)
      if (HB) {
        hB = hB && lx_confirm(tgB, s2B) && slot_valid(sB);
        HB = __ballot(hB);
      }
      if (!(HA | HB) && spUb < thr_r) return 1;   // the bound cut: nothing of the prefix is in the filter
      bool one_g = sp_one;
      if (!sp_one) {
        // several genes.  A list of several genes among the matches (the escape value): the usual order, whose rounds ask the
        // position table for such lists.  Else: one gene's single-gene lists only?
        if (!(HA | HB)) return 2;
        if (__ballot((hA & (pA == LTAB_ESC)) | (hB & (pB == LTAB_ESC)))) return 2;
        const uint32_t g = HA ? (uint32_t)__builtin_amdgcn_readlane((int)pA, (int)__builtin_ctzll(HA))
                              : (uint32_t)__builtin_amdgcn_readlane((int)pB, (int)__builtin_ctzll(HB));
        one_g = __ballot((hA & (pA != g)) | (hB & (pB != g))) == 0ull;
      }
      // (a few per cent of the reads) the matches in the usual order: slot s was probed by lane s / 2 of round A or B (even / odd
      // s < 2 nA - 1) or by lane s - nA of B; the T slots in front of the stop that the tiles displaced are not probed yet
      auto settle_round = [&](const int j, const uint32_t v) {
        const uint32_t sl = ln + 64u * (uint32_t)j;
        const bool eo = sl < 2u * nA - 1u, inB = sl < 128u - T;
        const uint32_t src = eo ? sl >> 1 : (inB ? sl - nA : sl - (128u - T));
        const uint32_t bit = eo ? sl & 1u : (inB ? 1u : 2u);
        const uint32_t pv = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src << 2), (int)v);
        mt[j] = ((pv >> bit) & 1u) != 0u;
        // (several genes: the matched entry's gene travels with its bit -- A's in bits 3..15, B's in 16..28, F's in a word of its own)
        slo[j] = sp_one ? P.lx_gene : ((bit == 0u ? pv >> 3 : pv >> 16) & LTAB_ESC);
        okm[j] = mt[j] ? 0xFFFFFFFFu : 0u;
      };
      const uint32_t vAB = (hA ? 1u : 0u) | (hB ? 2u : 0u) | (sp_one ? 0u : ((pA << 3) | (pB << 16)));
      settle_round(0, vAB);
      settle_round(1, vAB);
      if (HA | HB) {
        // the whole prefix is known now: what it covers (as the vote counts it) + the tiles -- a read with more errors than the
        // even slots forgive is settled here, behind the two rounds an off-target read costs
        const uint64_t H0 = __ballot(mt[0]), H1 = __ballot(mt[1]);
        const uint32_t cov = cover(H0, 0ull) + cover(H1, H0) + cover(0ull, H1) + k * (uint32_t)__builtin_popcountll(HA >> nA);
        if (one_g && cov >= thr_r && (sp_one || cov > spUb)) {
          write_the_gene(sp_one ? P.lx_gene : (uint32_t)__builtin_amdgcn_readfirstlane((int)(HA ? __builtin_amdgcn_readlane((int)pA, (int)__builtin_ctzll(HA))
                                                                                                   : __builtin_amdgcn_readlane((int)pB, (int)__builtin_ctzll(HB)))));
          return 1;
        }
      }
      // ... then the displaced slots, and on behind the cut's first stop as ever
      uint32_t pF = 0u, tgF = 0u, s2F = 0u;
      bool hF = lx_hit_at(128u - T + ln, ln < T, pF, tgF, s2F);
      if (__ballot(hF)) hF = hF && lx_confirm(tgF, s2F) && slot_valid(ln < T ? 128u - T + ln : 0u);
      if (!sp_one && __ballot(hF & (pF == LTAB_ESC))) return 2;
      settle_round(1, vAB | (hF ? 4u : 0u));
      if (!sp_one) {
        // (the displaced slots' genes: slot sl >= 128 - T of round 1 was probed by lane sl - (128 - T))
        const uint32_t sl = ln + 64u;
        const uint32_t pvF = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((sl >= 128u - T ? sl - (128u - T) : 0u) << 2), (int)pF);
        if (sl >= 128u - T) slo[1] = pvF & LTAB_ESC;
      }
      lane_any = mt[0] | mt[1];
      return 0;
    };
