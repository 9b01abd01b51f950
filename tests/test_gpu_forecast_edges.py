"""-m gpu: the forecast kernels (fd_forecast.hip) across the whole input range their entry points accept -- T in [2, 8], post in [1, 256]
(both sides of the trajectory-groups launch's dynamic-LDS opt-in), fd_forecast_groups up to its 8192-box limit, fd_nearest_rows across
its 256-thread reduction -- with exact ties, values exactly on the reject / match thresholds, and the count contract of
fd_forecast_from_detections (0, negative and over-post counts, sample independence, every output written, captured-graph replay).
Everything here is float64 index logic: every comparison is exact."""
import numpy as np
import pytest
import torch

from parity_util import report

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _edge_case(g, case):
    T = 1 + len(g[case + "_time"])
    centers = [g["%s_centers_%d" % (case, t)] for t in range(T)]
    velocity = [g["%s_velocity_%d" % (case, t)] for t in range(T)]
    return str(g[case + "_class"]), g[case + "_time"], centers, velocity


def _check_against_golden(g, case, got_tags, got_centres, got_ids=None):
    want_tags, want_centres = g[case + "_traj_tags"], g[case + "_traj_centers"]
    T = want_tags.shape[1]
    assert np.array_equal(np.asarray(got_tags, np.int64).reshape(-1, T), want_tags), case
    assert np.array_equal(np.asarray(got_centres, np.float64).reshape(-1, T, 3), want_centres), case
    if got_ids is not None:
        assert np.array_equal(np.asarray(got_ids, np.int64), g[case + "_traj_ids"]), case


# ------------------------------------------------------------------------------------------------ (a) the reference's tracker at the edges
def test_forecast_chains_match_reference_edges_golden(hip, golden):
    """fd_forecast_chains (single sweep) on every forecast_edges.npz case: forward / back-cast chains, constant-velocity roll-outs and
    match_boxes' indices identical to the reference's tracker and match_boxes; status 1 exactly for the cases with an empty step."""
    g = golden("forecast_edges.npz")
    for case in g["cases"]:
        cls, time, centers, velocity = _edge_case(g, case)
        T = len(centers)
        counts = np.array([len(c) for c in centers], np.int32)
        n = max(1, int(counts.max()))
        C, V = np.zeros((T, n, 3)), np.zeros((T, n, 3))
        for t in range(T):
            C[t, :counts[t]], V[t, :counts[t]] = centers[t], velocity[t]
        r = hip.forecast_chains(_dev(C), _dev(V), _dev(counts), _dev(np.asarray(time, np.float64)), 2.0 if cls == "car" else 1.0)
        r = {k: v.cpu().numpy() for k, v in r.items()}
        empty = bool((counts == 0).any())
        assert int(r["status"][0]) == int(empty), case
        if empty:
            assert not r["fwd_ok"].any() and not r["bwd_ok"].any(), case
            assert len(g[case + "_traj_tags"]) == 0
            continue
        n0, nl = int(counts[0]), int(counts[T - 1])
        fwd = [list(r["fwd_idx"][i]) for i in range(n0) if r["fwd_ok"][i]]
        bwd = [list(r["bwd_idx"][i][::-1]) for i in range(nl) if r["bwd_ok"][i]]
        tags = fwd + [[i] * T for i in range(n0)] + bwd
        centres = [[centers[t][j] for t, j in enumerate(ch)] for ch in fwd] + [list(r["cv_centers"][i]) for i in range(n0)] + \
                  [[centers[t][j] for t, j in enumerate(ch)] for ch in bwd]
        _check_against_golden(g, case, tags, centres)
        if case + "_match_tags" in g:
            assert np.array_equal(r["match_idx"][:, :n0], g[case + "_match_tags"]), case
    report("forecast chains vs reference tracker at the edges: %d cases identical" % len(g["cases"]), 0.0, 0.0)


def _packed_from_steps(centers_list, velocity_list, post):
    """head rows [T, post, 11] (x,y,z,w,l,h,vx,vy,yaw,score,label) carrying the given float32-exact centres / velocities"""
    T = len(centers_list)
    p = np.zeros((T, post, 11), np.float32)
    for t in range(T):
        n = len(centers_list[t])
        p[t, :n, :3] = centers_list[t]
        p[t, :n, 3:6] = 1.0
        p[t, :n, 6:8] = velocity_list[t][:, :2]
        p[t, :n, 9] = 0.5
        p[t, :n, 10] = t
        assert np.array_equal(p[t, :n, :3].astype(np.float64), centers_list[t]) and not velocity_list[t][:, 2].any()
    return p


def test_forecast_from_detections_matches_reference_edges_golden(hip, golden):
    """fd_forecast_from_detections on every forecast_edges.npz case as lidar-frame boxes (records = NULL), the cases of one (T, class)
    in one batch padded to their largest step: trajectories (kind order, box index per step, centres), n_traj, multi_future's forecast
    ids and match_boxes' indices identical to the reference's; status 1 and no trajectory exactly for the cases with an empty step."""
    from futuredet_amd import forecast

    g = golden("forecast_edges.npz")
    groups = {}
    for case in g["cases"]:
        cls, time, centers, velocity = _edge_case(g, case)
        groups.setdefault((len(centers), cls), []).append(case)
    n_checked = 0
    for (T, cls), cases in sorted(groups.items()):
        post = max(1, max(len(_edge_case(g, c)[2][t]) for c in cases for t in range(T)))
        packed = np.stack([_packed_from_steps(_edge_case(g, c)[2], _edge_case(g, c)[3], post) for c in cases])
        counts = np.array([[len(_edge_case(g, c)[2][t]) for t in range(T)] for c in cases], np.int32)
        time = np.stack([np.asarray(g[c + "_time"], np.float64) for c in cases])
        h = forecast.sweep_forecast(_dev(packed), _dev(counts), _dev(time), None, classname=cls).host()
        for b, case in enumerate(cases):
            got = forecast.trajectories_from_arrays(h, b)
            want_tags = g[case + "_traj_tags"]
            empty = bool((counts[b] == 0).any())
            assert int(h["status"][b]) == int(empty), case
            assert int(h["n_traj"][b]) == len(got) == len(want_tags), case
            if empty:
                assert (h["traj_kind"][b] == -1).all() and (h["traj_group"][b] == -1).all(), case
                continue
            n0 = int(counts[b, 0])
            kinds = [k for k, _, _, _ in got]
            nf = kinds.count(0)
            assert kinds == [0] * nf + [1] * n0 + [2] * (len(got) - nf - n0), case
            tags = [list(idx) if idx is not None else [int(h["traj_src"][b, j])] * T for j, (_, _, _, idx) in enumerate(got)]
            _check_against_golden(g, case, tags, [c for _, _, c, _ in got], [gid for _, gid, _, _ in got])
            if case + "_match_tags" in g:
                assert np.array_equal(h["match_idx"][b][:, :n0], g[case + "_match_tags"]), case
            n_checked += 1
    report("forecast from detections vs reference tracker + multi_future at the edges: %d cases" % n_checked, 0.0, 0.0)


# ------------------------------------------------------------------------------------------------ (b) every shape the ABI accepts
def _random_steps(rng, T, post, counts, chain=0):
    """per step float32-exact centres / velocities near common tracks; ``chain`` > 0 puts that many step-0 boxes 0.2 m apart on a line,
    in shuffled index order, so that one forecast group spans them and the label propagation needs many sweeps"""
    base = rng.uniform(-60, 60, (post, 3)) * [1, 1, 0.02]
    vel = rng.normal(0, 3, (post, 3)) * [1, 1, 0]
    cs, vs = [], []
    for t in range(T):
        n = int(counts[t])
        sel = rng.permutation(post)[:n]
        c = base[sel] + vel[sel] * 0.5 * t + rng.normal(0, 0.4, (n, 3)) * [1, 1, 0]
        if t == 0 and chain:
            c[:chain] = np.array([[10.0 + 0.2 * k, -20.0, -1.0] for k in rng.permutation(chain)])
        cs.append(c.astype(np.float32).astype(np.float64))
        vs.append((vel[sel] + rng.normal(0, 0.3, (n, 3)) * [1, 1, 0]).astype(np.float32).astype(np.float64))
    return cs, vs


def _oracle_trajectories(cls, time, cs, vs):
    """oracle.forecast's tracker + forecast_ids: [(kind, id, centres [T,3], index per step or None)] like trajectories_from_arrays"""
    from oracle import forecast as oforecast

    res = oforecast.tracker(cls, list(time), cs, vs)
    if res is None:
        return []
    fwd, cv, bwd = res
    T = len(cs)
    traj = [(0, np.stack([cs[t][j] for t, j in enumerate(ch)]), list(ch)) for ch in fwd] + [(1, cv[i], None) for i in range(len(cv))] + \
           [(2, np.stack([cs[t][j] for t, j in enumerate(ch)]), list(ch)) for ch in bwd]
    ids = oforecast.forecast_ids(np.stack([c[0] for _, c, _ in traj]))
    assert all(c.shape == (T, 3) for _, c, _ in traj)
    return [(k, int(i), c, idx) for (k, c, idx), i in zip(traj, ids)]


@pytest.mark.parametrize("T", [2, 8])
@pytest.mark.parametrize("post", [1, 224, 225, 256])
def test_forecast_from_detections_every_shape_vs_oracle(hip, T, post):
    """fd_forecast_from_detections at T in {2, 8} x post in {1, 224, 225, 256} (224 / 225: the last shape without and the first with the
    dynamic-LDS opt-in of the trajectory-groups launch), B = 3 (full counts, ragged counts, full counts with a long group of first
    boxes at post = 256): trajectory lists and indices, constant-velocity centres bit for bit, forecast ids exactly, against
    oracle/forecast.py on the head rows' own float64 values."""
    from futuredet_amd import forecast

    rng = np.random.default_rng(1000 * T + post)
    B = 3
    counts = np.array([[post] * T, rng.integers(1, post + 1, T), [post] * T], np.int32)
    chain = 64 if post == 256 else 0
    steps = [_random_steps(rng, T, post, counts[b], chain=chain if b == 2 else 0) for b in range(B)]
    packed = np.stack([_packed_from_steps(cs, vs, post) for cs, vs in steps])
    time = rng.uniform(0.4, 0.6, (B, T - 1))
    cls = "car" if T == 2 else "pedestrian"
    h = forecast.sweep_forecast(_dev(packed), _dev(counts), _dev(time), None, classname=cls).host()
    biggest = 0
    for b in range(B):
        want = _oracle_trajectories(cls, time[b], *steps[b])
        got = forecast.trajectories_from_arrays(h, b)
        assert int(h["status"][b]) == 0 and int(h["n_traj"][b]) == len(got) == len(want), b
        for j, ((gk, gid, gc, gidx), (wk, wid, wc, widx)) in enumerate(zip(got, want)):
            assert gk == wk and gid == wid, (b, j)
            assert np.array_equal(gc, wc), (b, j)  # chains: the boxes' own centres; roll-outs: c + t * v in float64, bit for bit
            assert (gidx is None) == (widx is None) and (gidx is None or list(gidx) == widx), (b, j)
        assert (h["traj_kind"][b, len(got):] == -1).all() and (h["traj_group"][b, len(got):] == -1).all()
        if want:
            biggest = max(biggest, int(np.bincount([i for _, i, _, _ in want]).max()))
    if chain:
        assert biggest >= chain, "the 0.2 m chain of first boxes is one group"
    report("forecast from detections T=%d post=%d vs oracle (largest group %d)" % (T, post, biggest), 0.0, 0.0)


# ------------------------------------------------------------------------------------------------ (c) the count contract
_PATTERNS = ("full", "zero@0", "zero@3", "zero@6", "neg@0", "neg@3", "neg@6", "over", "one", "ragged")


def _pattern_counts(rng, T, post):
    rows = {"full": [post] * T, "one": [1] * T, "ragged": list(rng.integers(1, post + 1, T)),
            "over": [post + 1, post, 2 ** 31 - 1, post + 40, post, 1000, post + 1]}
    for e in (0, 3, 6):
        rows["zero@%d" % e] = [post - 5] * T
        rows["zero@%d" % e][e] = 0
        rows["neg@%d" % e] = list(rows["zero@%d" % e])
        rows["neg@%d" % e][e] = -1
    return np.array([rows[p] for p in _PATTERNS], np.int32)


def _contract_batch():
    rng = np.random.default_rng(77)
    T, post = 7, 83
    counts = _pattern_counts(rng, T, post)
    B = len(counts)
    packed = np.zeros((B, T, post, 11), np.float32)
    for b in range(B):
        cs, vs = _random_steps(rng, T, post, [post] * T)
        packed[b] = _packed_from_steps(cs, vs, post)
    time = rng.uniform(0.4, 0.6, (B, T - 1))
    rec = np.zeros((B, 14))
    for b in range(B):
        q1, q2 = rng.normal(0, 1, 4), rng.normal(0, 1, 4)
        rec[b] = np.concatenate([q1 / np.linalg.norm(q1), rng.normal(0, 2, 3), q2 / np.linalg.norm(q2), rng.normal(0, 300, 3)])
    for e in (0, 3, 6):
        for a in (packed, time, rec):
            a[_PATTERNS.index("neg@%d" % e)] = a[_PATTERNS.index("zero@%d" % e)]
    return packed, counts, time, rec


def _fields(out):
    """host copies of the named ForecastOutputs views (never the alignment padding between them), compared as raw bytes"""
    return {name: a.copy() for name, a in out.host().items()}


def _assert_same(a, b, what, sample=None):
    for name in a:
        x, y = (a[name], b[name]) if sample is None else (a[name][sample[0]], b[name][sample[1]])
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), (what, name)


def test_forecast_from_detections_count_contract(hip):
    """One batch (T = 7, post = 83) whose samples carry full counts, a 0 and a -1 (circular NMS's undecided group) at step 0, 3 and 6,
    counts above post (up to INT_MAX), one box per step and ragged counts.  Every sample equals the same sample run alone; every output
    field is written (a 0x7F-filled and a zero-filled blob give the same named views); a count above post acts as post; a negative
    count is an empty step exactly like 0 -- status 1, n_traj 0, every traj_* entry -1, no chain kept."""
    from futuredet_amd import forecast, hip_ops

    packed, counts, time, rec = _contract_batch()
    B, T, post = counts.shape[0], counts.shape[1], packed.shape[2]
    P, C, TM, R = _dev(packed), _dev(counts), _dev(time), _dev(rec)
    out_ff = hip_ops.ForecastOutputs(B, T, post, P.device)
    out_ff.blob.fill_(0x7F)
    forecast.sweep_forecast(P, C, TM, R, classname="car", out=out_ff)
    out_00 = hip_ops.ForecastOutputs(B, T, post, P.device)
    forecast.sweep_forecast(P, C, TM, R, classname="car", out=out_00)
    batch = _fields(out_00)
    _assert_same(_fields(out_ff), batch, "0x7F-filled vs zero-filled outputs")
    for b, pat in enumerate(_PATTERNS):
        one = hip_ops.ForecastOutputs(1, T, post, P.device)
        one.blob.fill_(0x7F)
        forecast.sweep_forecast(P[b:b + 1], C[b:b + 1], TM[b:b + 1], R[b:b + 1], classname="car", out=one)
        _assert_same(batch, _fields(one), "sample %s in the batch vs alone" % pat, (b, 0))
        empty = pat.startswith("zero") or pat.startswith("neg")
        assert int(batch["status"][b]) == int(empty), pat
        if empty:
            assert int(batch["n_traj"][b]) == 0, pat
            for name in ("traj_kind", "traj_src", "traj_first", "traj_group"):
                assert (batch[name][b] == -1).all(), (pat, name)
            assert not batch["fwd_ok"][b].any() and not batch["bwd_ok"][b].any(), pat
        else:
            assert int(batch["n_traj"][b]) >= int(min(counts[b, 0], post)), pat
    for e in (0, 3, 6):
        _assert_same(batch, batch, "-1 at step %d is 0 at step %d" % (e, e), (_PATTERNS.index("neg@%d" % e), _PATTERNS.index("zero@%d" % e)))
    b = _PATTERNS.index("over")
    clipped = np.minimum(counts[b:b + 1], post)
    one = hip_ops.ForecastOutputs(1, T, post, P.device)
    forecast.sweep_forecast(P[b:b + 1], _dev(clipped), TM[b:b + 1], R[b:b + 1], classname="car", out=one)
    _assert_same(batch, _fields(one), "a count above post acts as post", (b, 0))
    report("forecast count contract: %d samples, batch = alone, all fields written, -1 = 0, > post = post" % B, 0.0, 0.0)


def test_forecast_graph_replay_with_every_count_pattern(hip):
    """sweep_forecast captured once in a graph with full counts, as FullSweepStep captures it; then the counts tensor is overwritten in
    place -- the whole mixed batch, then every pattern in every sample -- and the graph replayed: each replay equals the eager call."""
    from futuredet_amd import forecast, hip_ops

    packed, counts, time, rec = _contract_batch()
    B, T, post = counts.shape[0], counts.shape[1], packed.shape[2]
    P, TM, R = _dev(packed), _dev(time), _dev(rec)
    C = _dev(np.full((B, T), post, np.int32))
    out = hip_ops.ForecastOutputs(B, T, post, P.device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        forecast.sweep_forecast(P, C, TM, R, classname="car", out=out)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        forecast.sweep_forecast(P, C, TM, R, classname="car", out=out)
    trials = [("mixed", counts)] + [(p, np.repeat(counts[i:i + 1], B, axis=0)) for i, p in enumerate(_PATTERNS)]
    for name, cnt in trials:
        C.copy_(_dev(cnt))
        out.blob.fill_(0x7F)
        g.replay()
        torch.cuda.synchronize()
        eager = hip_ops.ForecastOutputs(B, T, post, P.device)
        forecast.sweep_forecast(P, _dev(cnt), TM, R, classname="car", out=eager)
        _assert_same(_fields(out), _fields(eager), "graph replay with counts %s vs eager" % name)
    report("forecast graph replay: %d count patterns, replay = eager" % len(trials), 0.0, 0.0)


# ------------------------------------------------------------------------------------------------ (d) fd_forecast_groups sizes
def _components(c, thresh):
    """connected components of the 'closer than thresh' graph numbered by smallest member.  Candidate pairs from a k-d tree, then the
    oracle's |a|^2 + |b|^2 - 2ab distance on each pair (no pair lies within 1e-9 of the threshold in these draws, so the rounding of
    the expansion cannot decide one)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree

    n = len(c)
    if n == 0:
        return np.zeros((0,), np.int32)
    pr = cKDTree(c).query_pairs(thresh + 1e-6, output_type="ndarray")
    a, b = c[pr[:, 0]], c[pr[:, 1]]
    d = np.sqrt(np.maximum((a * a).sum(1) + (b * b).sum(1) - 2 * (a * b).sum(1), 0.0))
    assert not (np.abs(d - thresh) < 1e-9).any()
    pr = pr[d < thresh]
    _, lab = connected_components(coo_matrix((np.ones(len(pr)), (pr[:, 0], pr[:, 1])), shape=(n, n)), directed=False)
    first = {}
    for i, l in enumerate(lab):
        first.setdefault(l, i)
    order = {l: r for r, l in enumerate(sorted(first, key=first.get))}
    return np.array([order[l] for l in lab], np.int32)


def _walk_clusters(rng, n):
    pts = []
    while len(pts) < n:
        p = rng.uniform(-50, 50, 3)
        for _ in range(int(rng.integers(1, 40))):
            pts.append(p.copy())
            p = p + rng.uniform(-0.12, 0.12, 3)
    c = np.asarray(pts[:n], np.float64).reshape(-1, 3)
    return c[rng.permutation(n)]


def test_forecast_groups_sizes_and_limit(hip):
    """fd_forecast_groups at n = 0, 1, 1023, 1024, 1025 (one box per thread, then a second one) and 8192 (its limit) on random-walk
    clusters, against the components of a k-d tree's candidate pairs (and oracle.forecast.forecast_ids up to n = 1025); an exact-tie case
    (boxes exactly 0.25 apart are not linked, 0.25 - 2^-26 apart are); n = 8193 is refused before any launch."""
    from oracle import forecast as oforecast

    rng = np.random.default_rng(31)
    for n in (0, 1, 1023, 1024, 1025, 8192):
        c = _walk_clusters(rng, n) if n else np.zeros((0, 3))
        got = hip.forecast_groups(_dev(c), 0.25).cpu().numpy()
        want = _components(c, 0.25)
        if n <= 1025:
            assert np.array_equal(oforecast.forecast_ids(c), want), n
        if n > 1:
            assert len(set(want.tolist())) < n, "some clusters"
        assert np.array_equal(got, want.astype(np.int32)), n
    d = 0.25 - 2.0 ** -26
    c = np.array([[0, 0, 0], [0.25, 0, 0], [0.5, 0, 0], [0, 0.25, 0], [0, 0, 0.25], [d, 0, 0], [1, 2, 0.5], [1.25, 2, 0.5], [1, 2.25, 0.5],
                  [1, 2, 0.75], [0, d, 0]], np.float64)
    want = oforecast.forecast_ids(c)
    assert want.tolist() == [0, 0, 1, 0, 2, 0, 3, 4, 5, 6, 0]  # 1 and 3 join 0 through their 0.25 - 2^-26 partners 5 and 10
    assert np.array_equal(hip.forecast_groups(_dev(c), 0.25).cpu().numpy(), want)
    with pytest.raises(hip.FutureDetHipError, match="8192"):
        hip.forecast_groups(_dev(np.zeros((8193, 3))), 0.25)
    report("forecast groups n = 0..8192 and the 0.25 tie identical to the oracle; n = 8193 refused", 0.0, 0.0)


# ------------------------------------------------------------------------------------------------ (e) fd_nearest_rows ties and sizes
@pytest.mark.parametrize("n_library", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("dim", [1, 30])
def test_nearest_rows_ties_and_sizes(hip, n_library, dim):
    """fd_nearest_rows against np.argmin of the float64 squared-difference sums.  Values are multiples of 1/8 in [-4, 4], so every sum
    is exact whatever the order or fusion, and equal sums are real ties: the lowest index must win.  Duplicated library rows sit where
    one thread holds them (j, j + 256, j + 512: thread j walks them in order) and where different threads do (j + 1, j + 129, j + 300:
    the cross-thread reduction decides)."""
    rng = np.random.default_rng(n_library * 100 + dim)
    lib = rng.integers(-32, 33, (n_library, dim)) / 8.0
    anchors = [j for j in (0, 7, 100, 200) if j < n_library]
    for j in anchors:
        for k in (256, 512, 1, 129, 300):
            if j + k < n_library:
                lib[j + k] = lib[j]
    queries = [lib[j] for j in anchors] + [lib[j] + rng.integers(-1, 2, dim) / 8.0 for j in anchors]
    queries += list(rng.integers(-32, 33, (64, dim)) / 8.0)
    if n_library > 1:
        queries.append(lib[n_library - 1])  # the last row (its earlier duplicates, if any, must win)
    q = np.array(queries, np.float64)
    d2 = ((lib[None, :, :] - q[:, None, :]) ** 2).sum(-1)
    want = np.argmin(d2, axis=1)
    got = hip.nearest_rows(_dev(lib), _dev(q)).cpu().numpy()
    assert np.array_equal(got, want.astype(np.int32)), np.nonzero(got != want)
    ties = int(((d2 == d2.min(1, keepdims=True)).sum(1) > 1).sum())
    if n_library > 1:
        assert ties > 0
    report("nearest rows n_library=%d dim=%d: %d queries, %d with tied minima" % (n_library, dim, len(q), ties), 0.0, 0.0)
