"""Dumps what a build computes on handles with known channels, for the bit-for-bit comparison of two builds
(profiles/known_channels_refactor.txt, item 4):

    python profiles/known_channels_dump.py --tree CHECKOUT --out DIR

CHECKOUT is a built checkout whose pyvb_amd is imported (this one by default; the parent commit's for the other side); only calls
that both have are used.  The problems are those of inputs_ref.CASES and CHANNEL_CASES and of regressors_ref.CASES and
CHANNEL_CASES (tests/), with their time splits and chain lengths, and two plain handles without known channels, one with
DiagonalGamma noise and one with Wishart noise.  Each handle runs two iterations in the reference bound mode and two in the exact
one, then the single entries in an order the iteration does not use -- update_B, update_E, the columns of A and C, Q, R, elbo --
and a set_inputs / set_regressors / set_observations on the handle that has run, with one more iteration behind it.  After every
step DIR/<handle>_<step>_<name>.npy holds every array of get_state(), get_input_state(), get_regressor_state(), the posterior
classes and the six parts of the bound per replicate.  `cmp` the two directories' files.
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=REPO)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, os.path.abspath(args.tree))
    import numpy as np
    import pyvb_amd
    import inputs_ref as IR
    import regressors_ref as RR
    from pyvb_amd import synth
    from pyvb_amd.lds import LDSBatch
    print("pyvb_amd from", os.path.dirname(pyvb_amd.__file__), "library version", pyvb_amd._capi.lib.pyvb_version(), flush=True)
    os.makedirs(args.out, exist_ok=True)
    count = [0]

    def save(name, step, b):
        out = dict(b.get_state())
        if b.P:
            out.update(b.get_input_state())
        if b.Pv:
            out.update(b.get_regressor_state())
        out["Sigma"], out["qld_x"] = b.get_posterior_classes()
        out["elbo"] = b.elbo()
        for k, v in sorted(out.items()):
            np.save(os.path.join(args.out, "%s_%s_%s.npy" % (name, step, k)), np.asarray(v))
            count[0] += 1

    def run(name, Y, U, V, st0, pri, lengths, split):
        b = LDSBatch.from_problem(Y, st0, pri, lengths=lengths, U=U, V=V)
        if split:
            b.set_time_split(split)
        for mode in ("reference", "exact"):
            b.set_bound_mode(mode)
            b.iterate(2)
            save(name, mode, b)
        if b.P:
            b.update_B()
        if b.Pv:
            b.update_E()
        b.update_columns("A", 0, b.D)
        b.update_columns("C", 0, b.D)
        b.update_Q()
        b.update_R()
        save(name, "entries", b)
        rng = np.random.default_rng(len(name))
        if b.P:
            b.set_inputs(U + 0.25 * rng.standard_normal(U.shape))
        if b.Pv:
            b.set_regressors(V + 0.25 * rng.standard_normal(V.shape))
        b.set_observations(Y + 0.25 * rng.standard_normal(Y.shape))
        b.iterate(1)
        save(name, "setters", b)
        b.close()

    for R, tag in ((IR, "in"), (RR, "rg")):
        for cases, problem, split_at in ((R.CASES, R.problem, 5 if R is IR else 6), (R.CHANNEL_CASES, R.channel_problem, -3)):
            for name in cases:
                prob = problem(name)
                Y, U, V, st0, pri, ln = (prob[:2] + (None,) + prob[2:5]) if R is IR else prob[:6]
                run("%s_%s" % (tag, name), Y, U, V, st0, pri, ln, cases[name][split_at])
    for noise in ("diagonal_gamma", "wishart"):
        Y, st0, pri = synth.make_problem(23, 5, 7, 3, seed=35400)
        pri = dict(pri, noise=noise)
        if noise == "wishart":      # v0 and a full w0 for each of the two noise nodes
            D, K = st0["A_mean"].shape[1], Y.shape[2]
            rng = np.random.default_rng(D + K)
            W = rng.standard_normal((D, D)); pri["Q_b0"] = 0.05 * (W @ W.T + D * np.eye(D)); pri["Q_a0"] = np.float64(0.5 * D + 1.0)
            W = rng.standard_normal((K, K)); pri["R_b0"] = 0.05 * (W @ W.T + K * np.eye(K)); pri["R_a0"] = np.float64(0.5 * K + 0.5)
        run("plain_" + noise, Y, None, None, st0, pri, None, None)
    print("wrote %d arrays to %s" % (count[0], args.out))


if __name__ == "__main__":
    main()
