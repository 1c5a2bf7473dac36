"""Host restatements of the launch arithmetic of the persistent-wave kernels (csrc/sk_pair_stream.h, csrc/sk_wave_common.h) -- TESTS ONLY,
shared by tests/test_fused_row_dealing.py (the plan before row-local dealing), tests/loss_batch_shapes.py (the loss launch's lane-group
chunks) and tests/test_adjoint_launch_plans.py / test_gpu_adjoint_launches.py (the fused adjoints' chunks, the one-draw plan).
No import of the package: everything is integer arithmetic on the arguments."""


def earlier_plan(P, NUp, L, lag, wpc, n_cu, pct, has_queue, G=1):
    """plan_pair_stream (sk_pair_stream.h), restated: P stream positions on waves of G lane groups with a stream each (G = 1: one
    stream position per wave and step -- the shared-y order, the plan before row-local dealing).  C0 / per count pairs per lane group."""
    max_waves = n_cu * wpc
    waves = min((P + G - 1) // G, max_waves)
    per = (P + waves * G - 1) // (waves * G)
    span = (L - 1 + lag + 24) // NUp + 2
    logC = 0
    while (span >> logC) + 1 > 3:
        logC += 1
    while ((per * (100 - pct) // 100) >> (logC + 1)) >= 24 and logC < 8:
        logC += 1
    queue = has_queue and waves == max_waves and per >= (8 << logC) and pct < 100
    if queue:
        C0, n_big, q_first = per * pct // 100, 0, waves * G * (per * pct // 100)
    else:
        base = P // (waves * G)
        rem = P - base * waves * G
        C0, n_big, q_first = base, (rem + G - 1) // G, P
        if base == 0:
            waves = n_big
    return dict(waves=waves, per=per, q_first=q_first, C0=C0, n_big=n_big, logC=logC, queue=int(queue))


# ---- the fused adjoints' chunk planner and the one-draw launch plan, as the launchers computed them before they shared one copy ---------
# (restated from launch_adj_fused_{linear,rbf}_rows, launch_amb, launch_df and launch_mb_one; tests/test_adjoint_launch_plans.py compares
# them with sk_plan_adjoint_chunks / sk_plan_one_draw)
def wave_group_wpb(lds_per_wave, n_waves, knob, dflt=4):
    """wave_group (sk_wave_common.h): waves per workgroup"""
    wpb = knob if knob > 0 else dflt
    wpb = max(1, min(4, wpb))
    while wpb > 1 and wpb * lds_per_wave > 160 * 1024:
        wpb -= 1
    while wpb > 1 and n_waves < wpb:
        wpb -= 1
    return wpb


def chunks_of(B, ppg):
    return (B + ppg - 1) // ppg if B > 0 else 1


def pick_chunk(A, B, max_groups):
    if B <= 0:
        return 1
    ppg = B
    for d in range(1, B + 1):
        if B % d == 0 and A * (B // d) <= max_groups:
            ppg = d
            break
    nch = max(1, min(B, max_groups // (A if A > 0 else 1)))
    return min((B + nch - 1) // nch, ppg)


def adjoint_chunks(A, B, G, NUp, n_cu, wpc, wpb_knob, lds_bytes, paired_form, force_nch=0):
    """The host arithmetic of a one-band fused adjoint's launch: pairs per lane-group chunk, pairs per lane group of a paired batch,
    rows per launch (0: one launch) and lane groups; None: refused by a 32-bit guard."""
    P = A * B if B > 0 else A
    max_groups = n_cu * wpc * G
    PPG = pick_chunk(A, B, max_groups)
    ppp = 1
    if B <= 0 and paired_form:
        ppp = max(1, min(64, P // max_groups))
        PPG = ppp
    rpl = 0
    if force_nch > 0:
        PPG = (B + force_nch - 1) // force_nch
    else:
        wpb = wave_group_wpb(lds_bytes, max_groups // G, wpb_knob)
        gpr = n_cu * wpb * G
        nr = max_groups // gpr if gpr > 0 and max_groups % gpr == 0 else 0
        nch = chunks_of(B, PPG)
        if B > 0 and nr >= 2 and not (A * nch == max_groups and nch % nr == 0 and B % nch == 0):
            single_rounds = (A * nch + max_groups - 1) // max_groups
            best = float(single_rounds) * float(PPG)
            m = nr
            while m <= B and m <= max_groups:
                if m >= nch and B % m == 0 and max_groups % m == 0 and B // m >= 4 * nr:
                    r = max_groups // m
                    launches = (A + r - 1) // r
                    t = 0.9 * float(launches) * float(B // m)
                    if A >= r and t < best * 0.97:
                        best, rpl, PPG = t, r, B // m
                m += nr
    if PPG > 0x3fffffff // NUp or P >= 0x7ff00000:
        return None
    groups = A * chunks_of(B, PPG) if B > 0 else (P + ppp - 1) // ppp
    return dict(PPG=PPG, ppp=ppp, rows_per_launch=rpl, groups=groups)


def waves_by_vgprs(waves_per_cu, vgprs):
    by_regs = 4 * (512 // ((vgprs + 7) & ~7))
    return max(1, min(waves_per_cu, by_regs))


def one_draw_waves_per_cu(lds_bytes, wpb0, vgprs, wpc_knob):
    """resident waves per CU of launch_amb / launch_df: whole workgroups of wpb0 waves by LDS, by registers, by the knob, at most 8"""
    wpc = waves_by_vgprs((160 * 1024) // (lds_bytes * wpb0) * wpb0, vgprs)
    if wpc_knob > 0 and wpc > wpc_knob:
        wpc = wpc_knob
    wpc = min(wpc, 8)
    if wpc >= wpb0:
        wpc = wpc // wpb0 * wpb0
    return max(wpc, 1)


def one_draw(P, max_waves, units, pct, ws_stride):
    """The share plan of a one-draw launch (one pair per wave at a time; units = bands x units per row): None: refused by a guard."""
    waves = min(P, max_waves)
    per = (P + waves - 1) // waves
    if P >= 0x7ff00000 or per > 0x1fffffff // units:
        return None
    ws_doubles = waves * ws_stride
    queue = waves == max_waves and per >= 8 and pct < 100
    if queue:
        C0 = per * pct // 100
        q_first = waves * C0
    else:
        waves = (P + per - 1) // per
        C0, q_first = per, P
    return dict(waves=waves, per=per, C0=C0, q_first=q_first, queue=int(queue), ws_doubles=ws_doubles)
