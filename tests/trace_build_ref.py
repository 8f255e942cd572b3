"""The build choice of launch_trace as it stood at commit 8c53523, BEFORE csrc/rt_trace_build.cpp existed: a transcription of that function's expressions
(csrc/rt_trace.hpp at 8c53523, line numbers below) and of KTrace::bits (748-750), not of rtl::trace_build.  tests/test_trace_build_host.py holds
rt.trace_build_cases to it over the whole domain.

Transcribed lines: 1024-1025 (stack entries, LDS bytes; launch_packets' 1070-1071 are the any-hit case), 1026 (qn), 1027 (fuse), 1028-1029 (impl), 1030-1032
(the arrays), 1041 (leafb) and the ladder 1042-1055.  A template argument of the ladder is written as the parent wrote it -- `ANY ? 2 : 0`, `!ANY` -- so
that the builds the ladder names for the other hit kind come out as what they were: the default build again.
"""

LEAFB4, STATS, COOP, NEAR, QN1, QN2, FUSE, IMPL, TIMING = 0x002, 0x004, 0x008, 0x010, 0x020, 0x040, 0x080, 0x100, 0x200   # RT_BUILD_*, include/rt_mi355.h
NODES = ("wnodesW", "wF", "iN2", "w4", "q4", "iN4", "iQ4")   # DevScene's members, in the order of RT_TRACE_NODES_*


def ktrace_bits(LEAFB=2, STATS_=False, COOP_=False, NEAR_=False, QN=0, FUSE_=False, IMPL_=False, TIMING_=False):
    """KTrace<Src, ANY, LEAFB, STATS, COOP, NEAR, QN, FUSE, IMPL, TIMING>::bits without RT_BUILD_LAUNCHED and the shift (745-750; the defaults are 745's)."""
    return ((LEAFB4 if LEAFB >= 4 else 0) | (STATS if STATS_ else 0) | (COOP if COOP_ else 0) | (NEAR if NEAR_ else 0) | (QN1 if QN == 1 else 0) |
            (QN2 if QN == 2 else 0) | (FUSE if FUSE_ else 0) | (IMPL if IMPL_ else 0) | (TIMING if TIMING_ else 0))


def launch_trace(ANY, stats, depth, anyStack, q4, wF, iN2, iN4, iQ4, timing, coop, nearFirst, qnodes, fused, impl_, leafb_any, leafbClosest):
    """-> (opt, nodes, implPairs, implLeafBoxes, stack, ldsBytes): `built` without LAUNCHED and the shift, the member `nodes` / `pairRecords` / `leafBoxes`
    point at, `stack`, `ldsBytes`.  stats: the launch's `stats` pointer is not null.  q4 .. iQ4: the scene's pointer is not null."""
    stack = max(4, ((anyStack if anyStack > 0 else 3 * ((depth + 1) // 2)) if ANY else depth))                                    # 1024
    ldsBytes = 256 * stack * (4 if ANY else 8)                                                                                    # 1025
    qn = ANY and qnodes != 0 and q4 and not stats and not nearFirst                                                               # 1026
    fuse = (not ANY) and fused != 0 and wF and not coop                                                                           # 1027
    impl = impl_ != 0 and (not stats or timing) and (                                                                             # 1028-1029
        (iN4 and (not qn or iQ4) and not nearFirst and leafb_any < 4 and not (qn and qnodes == 1) and anyStack > 0) if ANY else
        (not fuse and iN2 and not coop))
    nodes = (("iQ4" if qn else "iN4") if impl else ("q4" if qn else "w4")) if ANY else ("wF" if fuse else ("iN2" if impl else "wnodesW"))   # 1030
    implPairs = bool(impl)                                                                                                        # 1031
    implLeafBoxes = bool(ANY and impl)                                                                                            # 1032
    leafb = leafb_any if ANY else leafbClosest                                                                                    # 1041
    if stats and timing:                                                                                                          # 1042-1045
        built = ktrace_bits(2, False, False, False, 0, False, True, True) if impl else ktrace_bits(2, False, False, False, 0, False, False, True)
    elif impl and ANY:                                                                                                            # 1046
        built = ktrace_bits(2, False, False, False, 2 if ANY else 0, False, True) if qn else ktrace_bits(2, False, False, False, 0, False, True)
    elif impl:                                                                                                                    # 1047
        built = ktrace_bits(2, False, False, False, 0, False, True)
    elif stats and fuse:                                                                                                          # 1048
        built = ktrace_bits(2, True, False, False, 0, not ANY)
    elif stats:                                                                                                                   # 1049
        built = ktrace_bits(4, True) if leafb >= 4 else ktrace_bits(2, True)
    elif fuse:                                                                                                                    # 1050
        built = ktrace_bits(2, False, False, False, 0, not ANY)
    elif not ANY and coop:                                                                                                        # 1051
        built = ktrace_bits(2, False, not ANY)
    elif ANY and nearFirst:                                                                                                       # 1052
        built = ktrace_bits(2, False, False, ANY)
    elif qn and qnodes == 1:                                                                                                      # 1053
        built = ktrace_bits(2, False, False, False, 1 if ANY else 0)
    elif qn:                                                                                                                      # 1054
        built = ktrace_bits(2, False, False, False, 2 if ANY else 0)
    else:                                                                                                                         # 1055
        built = ktrace_bits(4, False) if leafb >= 4 else ktrace_bits(2, False)
    return built, NODES.index(nodes), implPairs, implLeafBoxes, stack, ldsBytes


def tune_from_env(env):
    """default_tune (100-110) and tune_from_env (114-129): the fields that choose a build, from a dict of environment variables."""
    atoi = lambda v: int(v)   # (every value the tests set is a plain decimal)
    t = dict(timing=0, coop=0, nearFirst=0, qnodes=-1, fused=0, impl=0, leafb=2, leafbClosest=2)   # 101
    for var, field in (("RT_TRACE_TIMING", "timing"), ("RT_IMPLICIT", "impl"), ("RT_FUSED", "fused")):   # 102, 107, 108
        if var in env:
            t[field] = atoi(env[var])
    if "RT_LEAFB" in env:                                                                                  # 118
        t["leafb"] = t["leafbClosest"] = atoi(env["RT_LEAFB"])
    if "RT_LEAFB_CLOSEST" in env:                                                                          # 119
        t["leafbClosest"] = atoi(env["RT_LEAFB_CLOSEST"])
    for var, field in (("RT_COOP", "coop"), ("RT_NEAR_FIRST", "nearFirst"), ("RT_QNODES", "qnodes")):    # 122, 123, 127
        if var in env:
            t[field] = atoi(env[var])
    return t
