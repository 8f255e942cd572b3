"""The ray-queue arithmetic of rt_wave_render as it stood at commit accc15b, BEFORE csrc/rt_wave_plan.cpp existed: a transcription of that function's
expressions (csrc/rt_wave.hip at accc15b, line numbers below), not of the planner.  tests/test_wave_plan_host.py holds rt.wave_plan to it.

Transcribed lines: 2165-2168 (slots per hit), 2187-2217 (bytes per hit, budget chunk, the three byte lambdas, n2_of), 2259-2260 (the 4 GiB comfort rule), 2282
(the 2^31-entries rejection), 2394-2395 (equal chunks), 2405 (room), and 2150 / 2182 (the per-frame arena).  The order of the arrays is the order in which
`carve` (2263-2281) and the pointer walk (2284-2292) took them.  Which of these applies when follows the control flow of 2297-2304, 2384 and 2399-2408.
"""

TOO_LARGE_MESSAGE = "ray queue chunk exceeds 2^31 entries; lower RT_QUEUE_BUDGET_MB"   # 2282
HIT_REC_BYTES = 12              # struct HitRec { uint32_t slot; float t; int tri; }  (line 48)
FRAME_ORDER = ("cand", "primT", "primTri", "hits", "pendC", "pendPos", "pendNrm", "pendMy")              # 2284-2292
RAYS_ORDER = ("shO", "shD", "shT", "aoOrg", "giD", "giOrg", "sh2O", "sh2D", "sh2T")                      # 2266-2270
RESULTS_ORDER = ("occ1", "giT", "giTri", "occ2", "occOvf", "giPos", "giHit")                             # 2273-2279 without RT_BIN_GI ...
RESULTS_ORDER_BIN_GI = ("occ1", "giT", "giTri", "occ2", "occOvf", "giPos", "giPerm", "giHit")            # ... and with it (2278)


def align_up(v, a):             # 2152
    return (v + a - 1) // a * a


def plan(slots, spp, ao, *, budget_bytes=16 << 30, bin_gi=False, chunks_from_slots=False, q2_predict=True, q2_cap=None, hits=None, share=0.0):
    """slots: nSlots (2165); spp, ao: SPP and A (2166-2167; ao = 0 when AO is off).  hits: *hostHits of 2387, None before the read-back; share: q2Share."""
    SPP, A = max(spp, 1), max(ao, 0)
    S1, S2 = A + 4 * SPP + 2, 6 * SPP                                                                    # 2168
    L1 = S1 - A                                                                                          # 2187
    gi_orgs = SPP if bin_gi else 1                                                                       # 2188
    per_hit = (L1 + S2) * 36 + (A + SPP) * 16 + ((1 if A > 0 else 0) + gi_orgs) * 16 + S1 + SPP * 12 + S2   # 2189
    ch_budget = align_up(min(slots, max(budget_bytes // per_hit, 4096)), 256)                            # 2190

    def rays_bytes(ch):                                                                                  # 2193-2196
        return (align_up(ch * L1 * 16, 256) + align_up(ch * S1 * 16, 256) + align_up(ch * L1 * 4, 256) + align_up(ch * 16, 256) +
                align_up(ch * SPP * 16, 256) + align_up(ch * gi_orgs * 16, 256) + 4096)

    def q2_bytes(n):                                                                                     # 2197
        return align_up(n * 6 * 16, 256) * 2 + align_up(n * 6 * 4, 256) + 4096

    def result_bytes(ch):                                                                                # 2199-2201
        return align_up(ch * S1, 256) + align_up(ch * SPP * 8, 256) + align_up(ch * S2, 256) * 2 + align_up(ch * SPP * 4, 256) * 3 + 4096

    def n2_of(ch, predict_q2):                                                                           # 2211-2216
        worst = ch * SPP
        n2 = max(int(2.0 * share * float(worst)) + 65536, worst // 32) if (q2_predict and predict_q2 and share > 0.0) else worst
        if q2_cap is not None:
            n2 = max(q2_cap, 64)
        return align_up(min(n2, worst), 64)

    def arena_bytes(ch, predict_q2):                                                                     # 2217
        return rays_bytes(ch) + q2_bytes(n2_of(ch, predict_q2))

    deferred = (not chunks_from_slots) and rays_bytes(ch_budget) + q2_bytes(ch_budget * SPP) > (4 << 30)   # 2259-2260
    too_large = ch_budget * max(S1, S2) >= (1 << 31)                                                     # 2282
    ch = room = ch_budget                                                                                # 2261, 2299: ensure(CH, CH)
    n_chunks = (slots + ch - 1) // ch                                                                    # 2304
    predict_q2 = False                                                                                   # 2209
    if hits is not None and (deferred or n_chunks > 1) and not chunks_from_slots:                        # 2384
        n_chunks = (hits + ch_budget - 1) // ch_budget                                                   # 2394
        if n_chunks > 0:
            ch = align_up((hits + n_chunks - 1) // n_chunks, 256)                                        # 2395
        predict_q2 = deferred                                                                            # 2400
        if deferred:
            room = ch_budget if n_chunks > 1 else min(ch_budget, align_up(ch + ch // 16, 256))           # 2405
            room = max(room, ch)                                                                         # 2219
    return dict(S1=S1, S2=S2, L1=L1, perHit=per_hit, chBudget=ch_budget, deferred=deferred, tooLarge=too_large, nChunks=n_chunks, ch=ch, room=room,
                q2Entries=n2_of(ch, predict_q2),
                frameBytes=slots * (4 + 4 + 4 + HIT_REC_BYTES + 16 + 4 + 8 + 8),                         # 2150, 2182
                raysBytes=arena_bytes(ch, predict_q2), raysAllocBytes=arena_bytes(room, predict_q2),     # 2241-2242
                resultsBytes=result_bytes(ch), resultsAllocBytes=result_bytes(room))                     # 2224-2225
