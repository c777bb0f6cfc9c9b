"""Generate tests/golden/per.npz from the reference's prioritized replay (PMatthaei/ma-league,
src/marl/components/replay_buffers/prioritized_replay_buffer.py: BinarySumTree, Memory).

TEST INFRASTRUCTURE ONLY. Usage: python tests/golden/make_per_golden.py <path to the reference's src directory>.
The reference's classes are loaded at run time and driven with seeded inputs; the file records DATA ONLY (inputs and
what the classes returned), no reference source text. The GPU box never sees the reference: it reads the .npz.

Per capacity C in (8, 64, 1024) (powers of two: BinarySumTree's leaves are then in slot order):
  c{C}.prio      [C] float64 priorities, multiples of 2^-10 so that every partial sum is exact in float64 and the
                 boundary draws below are exact ties; the last C // 4 slots of the `part` variant are never added
  c{C}.s         explicit s values: seeded uniforms over (0, total), every 7th cumulative boundary exactly (the tie
                 rule: s <= left goes left), 0 and the total
  c{C}.slot      the data index BinarySumTree.get(s) returned for each s, c{C}.p the leaf priority it returned
  c{C}.part.*    the same with only the first C - C // 4 slots added (a partially filled buffer)
  c{C}.mem.*     Memory.sample(n) with the module's random.uniform replaced by a recorded stream: the s values it drew
                 (s), the data indices (slot), the is_weight vector, beta after the call, n_entries and total
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def load_reference(src):
    # the module imports marl.components for the EpisodeBatch base of its buffer class, which this script never builds
    marl = types.ModuleType("marl")
    comps = types.ModuleType("marl.components")
    comps.EpisodeBatch = object
    marl.components = comps
    sys.modules.setdefault("marl", marl)
    sys.modules.setdefault("marl.components", comps)
    path = os.path.join(src, "marl", "components", "replay_buffers", "prioritized_replay_buffer.py")
    spec = importlib.util.spec_from_file_location("ref_per", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class RecordedUniform:
    """Stands in for the module's `random`: uniform(a, b) = a + (b - a) u_k for a seeded stream, and keeps what it gave."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.given = []

    def uniform(self, a, b):
        s = a + (b - a) * float(self.rng.random())
        self.given.append(s)
        return s


def tree_with(mod, cap, prio, filled):
    tree = mod.BinarySumTree(cap)
    for j in range(filled):
        tree.add(float(prio[j]))
    return tree


def explicit_s(rng, prio, filled):
    cum = np.cumsum(prio[:filled])
    total = float(cum[-1])
    s = list(rng.random(48) * total)
    s += [float(c) for c in cum[::7]]  # exact boundaries
    s += [0.0, total]
    return np.asarray(s, dtype=np.float64)


def main(src):
    mod = load_reference(src)
    out = {}
    for cap in (8, 64, 1024):
        rng = np.random.default_rng(1000 + cap)
        prio = rng.integers(1, 1001, size=cap).astype(np.float64) / 1024.0
        prio[rng.integers(0, cap)] = 900.0 * cap / 1024.0  # one heavy slot: several strata end in it
        out[f"c{cap}.prio"] = prio
        for tag, filled in (("", cap), (".part", cap - cap // 4)):
            tree = tree_with(mod, cap, prio, filled)
            s = explicit_s(rng, prio, filled)
            got = [tree.get(float(v)) for v in s]
            out[f"c{cap}{tag}.filled"] = np.int64(filled)
            out[f"c{cap}{tag}.s"] = s
            out[f"c{cap}{tag}.slot"] = np.asarray([g[2] for g in got], dtype=np.int64)
            out[f"c{cap}{tag}.p"] = np.asarray([g[1] for g in got], dtype=np.float64)
        # Memory.sample's weights for recorded draws
        mem = mod.Memory(cap)
        for j in range(cap):
            mem.tree.add(float(prio[j]))
        n = min(32, cap // 2)
        rec = RecordedUniform(2000 + cap)
        mod.random = rec
        beta0 = float(mem.beta)
        batch, idxs, w = mem.sample(n)
        out[f"c{cap}.mem.n"] = np.int64(n)
        out[f"c{cap}.mem.s"] = np.asarray(rec.given, dtype=np.float64)
        out[f"c{cap}.mem.slot"] = np.asarray(batch, dtype=np.int64)
        out[f"c{cap}.mem.is_weight"] = np.asarray(w, dtype=np.float64)
        out[f"c{cap}.mem.beta0"] = np.float64(beta0)
        out[f"c{cap}.mem.beta"] = np.float64(mem.beta)
        out[f"c{cap}.mem.increment"] = np.float64(mem.beta_increment_per_sampling)
        out[f"c{cap}.mem.n_entries"] = np.int64(mem.tree.n_entries)
        out[f"c{cap}.mem.total"] = np.float64(mem.tree.total())
    out["defaults"] = np.asarray([mod.Memory.e, mod.Memory.a, mod.Memory.beta, mod.Memory.beta_increment_per_sampling])
    # the priority rule on a few errors (Memory._get_priority)
    err = np.asarray([0.0, -0.5, 0.25, 3.0, 1e-3], dtype=np.float64)
    out["prio_rule.err"] = err
    out["prio_rule.p"] = np.asarray(mod.Memory(8)._get_priority(err), dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, "per.npz"), **out)
    print("wrote per.npz:", len(out), "arrays")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
