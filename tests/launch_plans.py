"""Host restatements of the launch arithmetic of the persistent-wave one-band kernels (csrc/sk_pair_stream.h) -- TESTS ONLY, shared by
tests/test_fused_row_dealing.py (the plan before row-local dealing) and tests/loss_batch_shapes.py (the loss launch's lane-group chunks).
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
