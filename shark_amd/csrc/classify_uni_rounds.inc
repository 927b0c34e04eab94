// classify_uni_rounds.inc -- a fragment of classify_uni_kernel's BODY (classify_uni.hpp includes it where it stands; not a header of its own):
// the rounds of a staged read: per-slot state, windows -> canonical k-mer -> XXH64 -> summary / table probes (probe_rounds), slot validity.
    uint64_t pos[U];
    uint32_t okm[U];   // all ones where the slot's probe has to be made, else 0
    uint4 bk[U];
    // each probe ends up with one word of its bucket: the low word of the slot that matched (mt[j] says whether one did)
    bool mt[U];
    uint32_t slo[U];
    bool lane_any = false;
    // REP: a bucket is reduced to that word right away (LDS-summary modes; table modes since the anchored extension fills mt / slo
    // from the reference as well).  WALK_ROUNDS: the instantiations with registers to spare (LDS-summary modes, 80+ VGPRs) walk all
    // their probes per round; the table modes walk probe by probe (the per-round form spilled there: 5-18 % slower on large indices)
#ifndef SHK_ROUNDS_ALL
#define SHK_ROUNDS_ALL 0
#endif
    constexpr bool WALK_ROUNDS = LSUM || SHK_ROUNDS_ALL;
    constexpr bool ROUNDS = LSUM || ANCH || SHK_ROUNDS_ALL;
    const uint4 *tab16 = reinterpret_cast<const uint4 *>(KT ? P.ktab : P.tab);
    // (the position table: as below, for the anchored extension's sample, which probes `atab` in every table mode)
    const uint32_t pmask = (uint32_t)((1ull << P.tab_lg) - 1ull) & (uint32_t)P.bf_mask;
    const uint32_t pspare = 1u << P.tab_lg;
    const uint32_t bmask = KT ? (uint32_t)((1ull << P.ktab_lg) - 1ull) : pmask;
    const uint32_t tagmask = (uint32_t)(P.bf_mask >> P.tab_lg);
    const uint32_t spare = KT ? (1u << P.ktab_lg) : pspare;
    const bool tab_stream = KT ? (P.ktab_nt != 0u) : (P.tab_nt != 0u);
    // the word a slot's high word is compared with (0 = empty slot): tag | valid | displacement 0
    auto want_for = [&](const uint64_t ps) -> uint32_t {
      const uint32_t tag = __builtin_amdgcn_alignbit((uint32_t)(ps >> 32), (uint32_t)ps, P.tab_lg) & tagmask;
      return (tag << 8) | 0x80u;
    };
    // (KT: pos[j] = the compared word << 32 | the home bucket; a key that left its home bucket is in the same bucket of a later line)
    auto want_of = [&](const int j) -> uint32_t { return KT ? (uint32_t)(pos[j] >> 32) : want_for(pos[j]); };
    auto bucket_of = [&](const int j, const uint32_t d) -> uint32_t { return ((uint32_t)pos[j] + (KT ? 8u * d : d)) & bmask; };
    // both orientations of the k-mer of slot (lane, j): x = its bases first-base-low (the fw stream's window), y = first-base-high
    // (the rv stream's window = the k-mer as kmer_utils.hpp:67-69 packs it); ~x is the reverse complement (kmer_utils.hpp:47-55)
    auto windows = [&](const int j, uint64_t &x, uint64_t &y) {
      const uint32_t qU = rcap - k - ((uint32_t)lane + 64u * (U - 1));
      const uint32_t sf = ((uint32_t)lane & 15u) << 1, sr = (qU & 15u) << 1;
      const uint32_t *f = fw + ((uint32_t)lane >> 4) + 4 * j;
      const uint32_t *r = rv + (qU >> 4) + 4 * (U - 1 - j);
      const uint32_t d0 = f[0], d1 = f[1], d2 = f[2];
      const uint32_t e0 = r[0], e1 = r[1], e2 = r[2];
      x = ((uint64_t)__builtin_amdgcn_alignbit(d2, d1, sf) << 32) | __builtin_amdgcn_alignbit(d1, d0, sf);
      y = ((uint64_t)__builtin_amdgcn_alignbit(e2, e1, sr) << 32) | __builtin_amdgcn_alignbit(e1, e0, sr);
    };
    // slot pp exists and all its k characters are valid (process_read, slot_ok)
    const uint64_t kmask0 = (1ull << k) - 1ull;
    auto slot_valid = [&](const uint32_t pp) -> bool {
      const bool exists = (TRO && !(SHK_TRO_ABL & 2)) ? ((pp < nk1e) | ((pp - P2) < nk2e)) : ((pp < nk1) | ((pp - P2) < nk2));
      if (!any_inv) return exists;
      const uint32_t V = pp >> 6, vs = pp & 63u;
      const uint64_t v0 = vbits[V], v1 = vbits[V + 1];
      const uint64_t win = (v0 >> vs) | ((v1 << 1) << (63u - vs));
      return exists & ((win & kmask0) == kmask0);
    };
    // ---- canonical k-mers, hashes, summary probes, table probes of the rounds [JLO, JHI) ----
    // (returns false when nothing of these rounds can have matched: no probe passed its summary / no slot is a valid k-mer)
    // known (table modes, anchored extension): bit j set = slot (lane, j) is settled already -- mt[j] / slo[j] stay, no probe is made
    auto probe_rounds = [&](auto lo_const, auto hi_const, const uint32_t known) -> bool {
      constexpr int JLO = decltype(lo_const)::value, JHI = decltype(hi_const)::value;
      constexpr bool ALL = JLO == 0 && JHI == U;   // the only phase: its caller ends the read when nothing can have matched
#pragma unroll
      for (int j = JLO; j < JHI; ++j) {
        uint64_t x, y;
        windows(j, x, y);
        const uint64_t fwd = y & kmer_mask, rc = ~x & kmer_mask;
        if (KT) {
          uint32_t hb, hw;
          ktab_home(fwd, rc, k, P.ktab_w, P.ktab_lg - 3u, hb, hw);
          pos[j] = ((uint64_t)hw << 32) | hb;
          continue;
        }
        const uint64_t canon = fwd < rc ? fwd : rc;         // KmerBuilder.hpp:49, ReadAnalyzer.hpp:55
        if (KX) { pos[j] = canon; continue; }               // (the table is keyed by the k-mer itself: no XXH64)
        const uint64_t hsh = xxh64_u64(canon);
        // (LDS-summary mode with a power-of-two size keeps the raw hash: every use below masks the bits it needs)
        pos[j] = POW2 ? (LSUM ? hsh : (hsh & P.bf_mask)) : bf_pos_np(hsh, P);
      }
      bool something = false;
      if (!LSUM) {
        // slot pp exists and all its k characters are valid; then the L2-resident summary
        bool ok[U];
#pragma unroll
        for (int j = JLO; j < JHI; ++j) {
          ok[j] = slot_valid((uint32_t)lane + 64u * j);
          if (ANCH) ok[j] = ok[j] & (((known >> j) & 1u) == 0u);
        }
        if (SUM) {
          uint32_t sw[U];
#pragma unroll
          for (int j = JLO; j < JHI; ++j) sw[j] = ok[j] ? P.sum32[(pos[j] >> P.sum_shift) >> 5] : 0u;
#pragma unroll
          for (int j = JLO; j < JHI; ++j) ok[j] = (sw[j] >> ((uint32_t)(pos[j] >> P.sum_shift) & 31u)) & 1u;
        }
        bool any = false;
#pragma unroll
        for (int j = JLO; j < JHI; ++j) { okm[j] = ok[j] ? 0xFFFFFFFFu : 0u; any |= ok[j]; }
        something = __ballot(any) != 0ull;
      } else if (KX) {
        // the exact table in LDS keyed by the canonical k-mer (kmer_table.hpp; pos[] is the k-mer): every entry is the one gene's,
        // none escapes to the position table
        // -- the candidate stage for every slot of the call, ONE ballot over them, the confirm stage behind it (see lx_probe)
        const uint8_t *img = reinterpret_cast<const uint8_t *>(lsum);
        bool any = false;
#if SHK_KX_ONE_STAGE
#pragma unroll
        for (int j = JLO; j < JHI; ++j) {
          mt[j] = kxtab_lookup(img, P.lsum_shift, P.kx_m2, pos[j]);
          any |= mt[j];
        }
#else
        uint32_t tg[U], s2[U];
#pragma unroll
        for (int j = JLO; j < JHI; ++j) {
          mt[j] = kxtab_candidate(img, P.lsum_shift, P.kx_m2, pos[j], tg[j], s2[j]);
          any |= mt[j];
        }
        if (__ballot(any)) {
          any = false;
#pragma unroll
          for (int j = JLO; j < JHI; ++j) {
            mt[j] = mt[j] & kxtab_confirm(img, tg[j], s2[j]);
            any |= mt[j];
          }
        }
#endif
#pragma unroll
        for (int j = JLO; j < JHI; ++j) {
          slo[j] = P.lx_gene;
          okm[j] = mt[j] ? 0xFFFFFFFFu : 0u;
        }
        lane_any |= any;
      } else if (LX) {
        // the exact table in LDS: displacement of the position's group, then the slot (shark_internal.hpp)
        const uint32_t *T = lsum;
        const char *D = reinterpret_cast<const char *>(lsum + LTAB_T_WORDS);
        const uint32_t tagmask15 = (uint32_t)(P.bf_mask >> LTAB_SLOT_LG);
        const uint32_t gmask2 = (tagmask15 & ((1u << LTAB_GROUP_LG) - 1u)) << 1;   // (pos[] is the raw hash: only the filter's bits count)
        uint32_t dd[U], ee[U], tg[U];
#pragma unroll
        for (int j = JLO; j < JHI; ++j) {
          dd[j] = *reinterpret_cast<const uint16_t *>(D + (((uint32_t)pos[j] >> (LTAB_SLOT_LG - 1)) & gmask2));
          tg[j] = __builtin_amdgcn_alignbit((uint32_t)(pos[j] >> 32), (uint32_t)pos[j], LTAB_SLOT_LG) & tagmask15;
        }
#pragma unroll
        for (int j = JLO; j < JHI; ++j) {
          const uint32_t base = (uint32_t)pos[j] + (tg[j] >> LTAB_GROUP_LG) * P.lsum_shift;   // (lds_table.hpp: the bits above the group spread the slots; lsum_shift = the multiplier)
          ee[j] = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(T) + (((base + dd[j]) << 2) & ((LTAB_T_WORDS - 1u) << 2)));
        }
        bool esc = false, any = false;
#pragma unroll
        for (int j = JLO; j < JHI; ++j) {
          mt[j] = (ee[j] >> 13) == ((tg[j] << 1) | 1u);
          slo[j] = ee[j] & LTAB_ESC;
          okm[j] = mt[j] ? 0xFFFFFFFFu : 0u;
          any |= mt[j];
          esc |= mt[j] & (slo[j] == LTAB_ESC);
        }
        // a multi-gene list (or a gene id beyond 13 bits) is not in the entry: the position table answers for these rounds
        something = __ballot(esc) != 0ull;
        if (!something) lane_any |= any;
      } else {
        uint32_t si[U], sw[U];
#pragma unroll
        for (int j = JLO; j < JHI; ++j) {
          si[j] = __builtin_amdgcn_alignbit((uint32_t)(pos[j] >> 32), (uint32_t)pos[j], P.lsum_shift);   // low LSL bits = summary index
          sw[j] = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(lsum) + ((si[j] >> 3) & (UG::SUM_BITS / 8 - 4)));
        }
        uint32_t any = 0;
#pragma unroll
        for (int j = JLO; j < JHI; ++j) {
          okm[j] = (uint32_t)__builtin_amdgcn_sbfe((int)sw[j], si[j], 1u);   // v_bfe_i32: bit (si & 31), sign extended
          any |= okm[j];
        }
        something = __ballot(any != 0u) != 0ull;
      }
      if (something) {
        // ---- position table: the probes that passed read their home bucket, the others the spare empty bucket ----
#pragma unroll
        for (int j = JLO; j < JHI; ++j) {
          const uint32_t bb = (uint32_t)pos[j] & bmask;
          const uint32_t bi = (bb & okm[j]) | (spare & ~okm[j]);
          if (!LSUM && tab_stream) {   // a table far beyond the caches: streaming loads (49.8 -> 54.6 G lookups/s, tools/gather_bench)
            const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(tab16) + bi);
            bk[j] = make_uint4(v.x, v.y, v.z, v.w);
          } else {
            bk[j] = load_bucket<LSUM && UNI>(tab16, bi);   // (the ragged instantiation runs out of registers with the short addresses)
          }
        }
        bool lane_more = false;
        bool more[U];
#pragma unroll
        for (int j = JLO; j < JHI; ++j) {
          const uint32_t want = want_of(j);
          const bool m0 = bk[j].y == want, m1 = bk[j].w == want;
          if (ROUNDS) {
            const bool kn = ANCH && ((known >> j) & 1u) != 0u;   // (a settled slot read the spare bucket: nothing matched)
            mt[j] = kn ? mt[j] : (m0 | m1);
            slo[j] = kn ? slo[j] : (m0 ? bk[j].x : bk[j].z);
          }
          lane_any |= m0 | m1;
          more[j] = !(m0 | m1) & ((bk[j].x & TAB_OVERFLOW) != 0u);   // some key of this home bucket lives further down the path
          lane_more |= more[j];
        }
        if (__ballot(lane_more) && !SHK_ABL(P, 8u)) {   // (ablation 8: no walks)
          // rare: the key may sit behind its (full) home bucket
          if (WALK_ROUNDS) {
            // round d looks at bucket home+d of every probe that is still searching, all loads in flight together (the
            // others read the spare bucket: one line for the wave) -- a memory round trip per displacement, not per probe
            uint32_t d = 0;
            do {
              ++d;
#pragma unroll
              for (int j = JLO; j < JHI; ++j) bk[j] = load_bucket<LSUM && UNI>(tab16, more[j] ? bucket_of(j, d) : spare);
              lane_more = false;
#pragma unroll
              for (int j = JLO; j < JHI; ++j) {
                const uint32_t want = KT ? want_of(j) : (want_of(j) | d);   // (a slot of the position table carries its displacement)
                const bool n0 = bk[j].y == want, n1 = bk[j].w == want;
                const bool found = more[j] & (n0 | n1);
                const bool ends = (bk[j].y == 0u) | (bk[j].w == 0u) | (d >= 63u);   // a free slot ends every search
                slo[j] = found ? (n0 ? bk[j].x : bk[j].z) : slo[j];
                mt[j] |= found;
                lane_any |= found;
                more[j] = more[j] & !found & !ends;
                lane_more |= more[j];
              }
            } while (__ballot(lane_more));
          } else {
            bool walked[U];
#pragma unroll
            for (int j = JLO; j < JHI; ++j) walked[j] = more[j];
            walk_probe_paths<U, !KT>(tab16, bk, more, lane_any, want_of, bucket_of, (uint32_t)JLO, (uint32_t)JHI);   // (a key found is moved into bk[j] in home form)
            if (ROUNDS) {
#pragma unroll
              for (int j = JLO; j < JHI; ++j) {
                const bool f = walked[j] & (bk[j].y == want_of(j));
                mt[j] |= f;
                slo[j] = f ? bk[j].x : slo[j];
              }
            }
          }
        }
      } else if (!LX && !ALL) {
        // nothing of these rounds passed the summary: no matches (the hit path may still run for the other rounds)
#pragma unroll
        for (int j = JLO; j < JHI; ++j) {
          if (ROUNDS) {
            const bool kn = ANCH && ((known >> j) & 1u) != 0u;   // (settled slots stay)
            mt[j] = kn && mt[j];
            slo[j] = kn ? slo[j] : 0u;
          } else bk[j] = make_uint4(0u, 0u, 0u, 0u);   // (an empty slot's compared word is 0: matches nothing)
        }
      }
      return LX || something;
    };
