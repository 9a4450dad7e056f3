"""Shared by the CPU and GPU tests of GPI_HDP.include_sample: drive the mirror as hdpgpc/tests/test_online.py:41-83 drives the
reference and compare, beat by beat, with the trace tests/golden/make_golden.py::gen_include_sample recorded there."""
import numpy as np


def _mirror(g, max_models=100):
    """The mirror set up as hdpgpc/tests/test_online.py sets up the reference, with the fixture's injected kernel parameters."""
    import hdpgpc.GPI_HDP as hdpgp

    std, std_dif, bs0, bs1, bg0, bg1 = (float(v) for v in g["estimators"])
    data = np.asarray(g["y"], dtype=np.float64)[:, :, None]
    xb = np.arange(float(data.shape[1]))[:, None]
    sw = hdpgp.GPI_HDP(xb, x_basis_warp=xb[::2], n_outputs=1, kernels=None, model_type="dynamic", ini_lengthscale=3.0,
                       bound_lengthscale=(1.0, 20.0), ini_gamma=std_dif, ini_sigma=std, ini_outputscale=300.0, noise_warp=std * 0.1,
                       bound_sigma=(bs0, bs1), bound_gamma=(bg0, bg1), bound_noise_warp=(std * 0.01, std * 0.02), warp_updating=False,
                       method_compute_warp="greedy", verbose=False, hmm_switch=True, max_models=max_models, mode_warp="rough",
                       bayesian_params=True, inducing_points=False, estimation_limit=None, free_deg_MNIV=20)
    sw.fixed_theta = tuple(float(v) for v in g["theta_inject"])
    return sw, xb, data


def _beat(sw):
    return (sw.actual_state, sw.M, sw.resp_assigned[-1].numpy().astype(np.int16), sw.q[-1].cpu().numpy().copy(),
            np.array([len(m.indexes) for m in sw.gpmodels[0]]))


def run_online(g, n=None):
    """The first n beats of the trace g (all of them by default).  A trace with the key x_shift hands beat i over on the grid
    x_basis + x_shift[i]: a non-zero shift takes the beat off the basis grid (make_golden.py gen_include_sample, off_grid)."""
    sw, xb, data = _mirror(g)
    shift = g["x_shift"] if "x_shift" in getattr(g, "files", g) else np.zeros(data.shape[0])
    tr = []
    for i in range(data.shape[0] if n is None else n):
        sw.include_sample(xb + float(shift[i]), data[i], with_warp=False)
        tr.append(_beat(sw))
    return sw, tr


# the two runs of tests/golden/include_sample_r102_forced_mirror.npz: (beats, max_models, force_model per beat)
FORCED_RUNS = {"cap": (14, 4, {}), "force": (12, 100, {6: 1, 7: 1, 9: 0})}


def run_forced(g, run):
    """One of FORCED_RUNS on the first beats of g (include_sample_r102_n40.npz): the model cap or a caller's force_model decides
    some beats.  Returns (sw, trace as run_online's, forced [n] bool).  A beat was forced when include_sample did not sort the
    clusters by size (it skips reorder() exactly on its forced no-birth branch)."""
    n, max_models, force = FORCED_RUNS[run]
    sw, xb, data = _mirror(g, max_models)
    calls, sort = [0], sw.reorder

    def counted(*a):
        calls[0] += 1
        return sort(*a)

    sw.reorder = counted
    tr, forced = [], []
    for i in range(n):
        calls[0] = 0
        sw.include_sample(xb, data[i], with_warp=False, force_model=force.get(i))
        tr.append(_beat(sw))
        forced.append(calls[0] == 0)
    return sw, tr, np.array(forced)


def record_forced_mirror(g, path):
    """Write include_sample_r102_forced_mirror.npz: THIS PROJECT'S OWN behaviour on the forced path (the reference raises
    UnboundLocalError there, GPI_HDP.py:2187), recorded on the CPU tier (cpu_double.install) in compare_online's format, one key
    prefix per run of FORCED_RUNS."""
    out = {}
    for run in FORCED_RUNS:
        _, tr, forced = run_forced(g, run)
        out[f"{run}_state"], out[f"{run}_M"] = np.array([b[0] for b in tr]), np.array([b[1] for b in tr])
        out[f"{run}_forced"] = forced
        for i, (_, _, labels, q, counts) in enumerate(tr):
            out[f"{run}_b{i}_labels"], out[f"{run}_b{i}_q"], out[f"{run}_b{i}_counts"] = labels, q, counts
    np.savez_compressed(path, **out)


def compare_forced(g, rec, tol):
    """Replay both FORCED_RUNS against the recorded fixture rec: the forced beats and every decision identical, q within tol."""
    for run in FORCED_RUNS:
        _, tr, forced = run_forced(g, run)
        assert np.array_equal(forced, rec[f"{run}_forced"]), f"run {run}: forced beats {forced} vs {rec[f'{run}_forced']}"
        compare_online({k[len(run) + 1:]: rec[k] for k in rec.files if k.startswith(run + "_")}, tr, tol)


def compare_online(g, tr, tol):
    """Per beat: the chosen cluster, the number of clusters, the assignments of the whole history and the cluster sizes must
    be IDENTICAL to the reference's; the score matrix within tol (entries that are -inf there must be -inf here)."""
    from conftest import _note

    worst = 0.0
    for i, (state, M, labels, q, counts) in enumerate(tr):
        assert state == int(g["state"][i]) and M == int(g["M"][i]), f"beat {i}: cluster {state} of {M}, reference {g['state'][i]} of {g['M'][i]}"
        assert np.array_equal(labels, g[f"b{i}_labels"]), f"beat {i}: assignments of the history differ"
        assert np.array_equal(counts, g[f"b{i}_counts"]), f"beat {i}: cluster sizes {counts} vs {g[f'b{i}_counts']}"
        ref = g[f"b{i}_q"]
        assert q.shape == ref.shape and np.array_equal(np.isinf(q), np.isinf(ref)), f"beat {i}: score matrix layout"
        fin = np.isfinite(ref)
        if fin.any():
            worst = max(worst, float(np.max(np.abs(q[fin] - ref[fin]) / np.maximum(np.abs(ref[fin]), 1e-300))))
    _note(worst)
    assert worst <= tol, f"worst relative error of the score matrices {worst:.3e} > {tol:.1e}"
    return worst
