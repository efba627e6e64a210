"""What tests/tools/make_golden_ik_edges.py (the generator), tests/test_ik_edges_cpu.py and tests/test_ik_edges_gpu.py share:
the names behind the `category` column of tests/golden/ik_edges_<env>.npz, the conditions a fixture has to meet, and the
comparison of one implementation's answers (the C oracle's or the device's) with the recorded SciPy rows.  NumPy only."""
import os

import numpy as np

CATEGORIES = ["pressed", "far", "on_bound", "near_bound", "still", "big_rotation", "infeasible", "capped"]
CAPS = [1, 2, 3, 5, 8, 13, 21, 64]      # max_nfev of the capped rows; every other row has 0 = least_squares' default, 100 n
N_KEEP = 48                             # kept rows per category and model
SENS_MAX = 1e-9                         # a case is kept if SciPy's own result moves by no more than this under the re-runs
MAX_DROP = {"far": 0.40}                # share of dropped candidates; every other category: 0.10
ON_BOUND = 1e-9                         # n_on_bound counts result components within this of a bound
PRESSED = 1e-20

IK_TOL = 1e-6                           # rad, against SciPy: the project's bar (tests/test_oracle_ik.py, test_gpu_parity.py)
NFEV_SLACK = 3                          # per 48 rows of a category: rows whose nfev may differ, and then by exactly 1

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "golden")


def load(env):
    return np.load(os.path.join(GOLDEN, "ik_edges_%s.npz" % env))


def arm_mask(cm, arm):
    return np.array(list(cm.desc.arm_q_id[arm])[:cm.desc.arm_nq[arm]])


def bound_distance(cm, arm, q):
    """Distance of every component of an arm's q to its nearer bound (negative outside)."""
    rg = np.array([l["joint"]["range"] for l in cm.asset["links"]], dtype=float)[arm_mask(cm, arm)]
    return np.minimum(q - rg[:, 0], rg[:, 1] - q)


def check_fixture(env, cm, g):
    """The conditions of one model's fixture; the generator asserts them before it writes the file."""
    cat, narms = g["category"], sum(bool(cm.desc.arm_present[a]) for a in range(2))
    assert list(g["category_names"]) == CATEGORIES
    assert (g["sens"] <= SENS_MAX).all()
    for c, name in enumerate(CATEGORIES):
        m = cat == c
        kept, dropped = int(g["kept"][c]), int(g["dropped"][c])
        assert m.sum() == kept >= N_KEEP, (env, name, m.sum(), kept)
        assert dropped / (kept + dropped) <= MAX_DROP.get(name, 0.10), (env, name, kept, dropped)
        assert len(set(g["arm"][m].tolist())) == narms, (env, name)
        caps = set(g["max_nfev"][m].tolist())
        assert caps == (set(CAPS) if name == "capped" else {0}), (env, name, caps)
    for i in range(len(cat)):
        n = cm.desc.arm_nq[int(g["arm"][i])]
        dist = bound_distance(cm, int(g["arm"][i]), g["q_out"][i][:n])
        assert g["n_on_bound"][i] == (dist <= ON_BOUND).sum() and g["min_dist"][i] == dist.min()
    far, pressed, bad = cat == CATEGORIES.index("far"), cat == CATEGORIES.index("pressed"), cat == CATEGORIES.index("infeasible")
    assert (g["status"][far] == 0).sum() >= 2 and (g["n_on_bound"][far] > 0).sum() >= 10, env
    assert (g["min_dist"][pressed] <= PRESSED).sum() >= 10, env
    assert (g["status"][bad] == -2).all() and (g["nfev"][bad] == 0).all() and (g["status"][~bad] >= 0).all()
    hit = g["status"] == 0                                   # stopped by the cap and by nothing else
    cap = np.where(g["max_nfev"] > 0, g["max_nfev"], 100 * np.array([cm.desc.arm_nq[int(a)] for a in g["arm"]]))
    assert (g["nfev"][hit] == cap[hit]).all() and (g["nfev"] <= cap).all()


def groups(g):
    """(arm, max_nfev, row indices): the rows one batched call, or one compiled model, can take."""
    for arm in sorted(set(g["arm"].tolist())):
        for cap in sorted(set(g["max_nfev"].tolist())):
            idx = np.where((g["arm"] == arm) & (g["max_nfev"] == cap))[0]
            if len(idx):
                yield arm, cap, idx


def compare(cm, g, q, qpos_after, nfev, status, who):
    """Asserts one implementation's answers to every row against the recorded SciPy rows; q is padded to 7 like q_out.
    Prints and returns the worst |q - q_scipy| per category."""
    assert np.isfinite(q).all() and np.isfinite(qpos_after).all()
    dq = np.abs(q - g["q_out"]).max(axis=1)
    da = np.abs(qpos_after - g["qpos_after"]).max(axis=1)
    worst = {}
    for c, name in enumerate(CATEGORIES):
        m = g["category"] == c
        worst[name] = max(dq[m].max(), da[m].max())
        off = nfev[m] != g["nfev"][m]
        print("%s %-13s worst %.1e  nfev off by one: %d of %d" % (who, name, worst[name], off.sum(), m.sum()))
    for c, name in enumerate(CATEGORIES):
        m = g["category"] == c
        assert worst[name] < IK_TOL, (who, name, worst[name])
        assert np.array_equal(status[m], g["status"][m]), (who, name, np.where(m)[0][status[m] != g["status"][m]])
        off = nfev[m] != g["nfev"][m]
        assert off.sum() <= NFEV_SLACK * m.sum() // N_KEEP and (np.abs(nfev[m] - g["nfev"][m])[off] == 1).all(), (who, name, off.sum())
    bad = g["status"] == -2                                  # "IK failed": nothing evaluated, nothing written
    assert (nfev[bad] == 0).all() and np.array_equal(qpos_after[bad], g["qpos"][bad])
    capped = g["max_nfev"] > 0
    hit = capped & (g["status"] == 0)                        # SciPy was stopped by the cap: so is the implementation, after k
    assert np.array_equal(nfev[hit], g["max_nfev"][hit]) and (status[hit] == 0).all()
    assert (nfev[capped] <= g["max_nfev"][capped]).all()
    return worst
