"""tests/mc_model.py with samples that are not from the present (-eI): the same independent statement of the model, with
one more key in the model dictionary.

TEST INFRASTRUCTURE (numpy and the standard library only; nothing from the device, the oracle or the reference).

Model: everything of tests/mc_model.py (its lines 13-52), and
  * sample i enters at sample_times[i] generations, in sample_pops[i]; below that time its lineage does not exist: no
    recombination and no mutation on it, nobody coalesces into it, and it is no partner and no migrant;
  * a sample time is the start of an epoch (an entry of change_times), the smallest is 0, and the times ascend with the
    sample index (what the front-end of the program writes);
  * a join (single_mig) at the start of an epoch moves the lineages that exist already; a sample that enters at that same
    epoch start enters in sample_pops[i] as given.
The tree at position 0 is the structured coalescent of these serial samples: lineages enter at their times, in index
order.  Everything along the sequence is mc_model.ARG's own code, which reads the leaf heights where it needs them: the
cut is uniform on the length that exists, candidates are `height[v] <= t < height[parent]`, the emission takes branch
lengths from the heights.  With all times zero the draws are mc_model.ARG's, random number for random number.
"""
import random

import numpy as np

import mc_model
from mc_model import INF, fastexp, prepare_rows, summarise, no_rows  # noqa: F401


class Model(mc_model.Model):
    def __init__(self, m):
        super().__init__(m)
        st = m.get("sample_times")
        self.stime = [float(t) for t in st] if st is not None else [0.0] * self.n
        assert len(self.stime) == self.n
        assert min(self.stime) == 0.0, "the smallest sample time must be 0"
        assert all(a <= b for a, b in zip(self.stime, self.stime[1:])), "sample times must ascend with the sample index"
        assert all(t in self.T for t in self.stime), "a sample time must be the start of an epoch"


class ARG(mc_model.ARG):
    """mc_model.ARG with the serial-sample tree at position 0"""

    def _initial_tree(self):
        m, rng, st = self.m, self.rng, self.stat
        n, P = m.n, m.P
        self.height = list(m.stime) + [0.0] * (n - 1)
        self.parent = [-1] * (2 * n - 1)
        self.child = [None] * (2 * n - 1)
        self.pop0 = list(m.spop) + [0] * (n - 1)
        self.path = [[] for _ in range(2 * n - 1)]
        live = [i for i in range(n) if m.stime[i] <= 0.0]
        pending = [i for i in range(n) if m.stime[i] > 0.0]       # ascending in time, as the indices are
        cur = [m.spop[i] for i in live]          # current population of every live lineage
        t, e, nxt = 0.0, 0, n
        while len(live) > 1 or pending:
            kp = [0] * P
            for q in cur:
                kp[q] += 1
            rc = [kp[p] * (kp[p] - 1) / 2.0 / (2.0 * m.N[e][p]) for p in range(P)]
            rm = [kp[p] * m.mtot[e][p] for p in range(P)]
            lam = sum(rc) + sum(rm)
            dt = rng.expovariate(lam) if lam > 0 else INF
            end = m.epoch_end(e)
            hit = t + dt < end
            t1 = t + dt if hit else end
            assert t1 < INF, "no coalescence is possible any more"
            for p in range(P):
                st[self.o_co + e * P + p] += kp[p] * (kp[p] - 1) / 2.0 * (t1 - t)
                st[self.o_mo + e * P + p] += kp[p] * (t1 - t)
            t = t1
            if not hit:
                e += 1
                for i, v in enumerate(live):
                    q = m.jmap[e][cur[i]]
                    if q != cur[i]:
                        cur[i] = q
                        self.path[v].append((t, q))
                while pending and m.stime[pending[0]] == t:          # after the join: they enter where they are said to be
                    v = pending.pop(0)
                    live.append(v); cur.append(m.spop[v])
                continue
            u = rng.random() * lam
            done = False
            for p in range(P):
                if u < rc[p]:
                    idx = [i for i in range(len(live)) if cur[i] == p]
                    i, j = rng.sample(idx, 2)
                    a, b = live[i], live[j]
                    self.height[nxt] = t
                    self.pop0[nxt] = p
                    self.parent[a] = self.parent[b] = nxt
                    self.child[nxt] = [a, b]
                    for k in sorted((i, j), reverse=True):
                        del live[k]; del cur[k]
                    live.append(nxt); cur.append(p)
                    nxt += 1
                    st[self.o_cc + e * P + p] += 1
                    done = True
                    break
                u -= rc[p]
            if done:
                continue
            for p in range(P):
                if u < rm[p]:
                    idx = [i for i in range(len(live)) if cur[i] == p]
                    i = idx[min(int(u / m.mtot[e][p]), len(idx) - 1)]
                    q = self._mig_target(e, p)
                    cur[i] = q
                    self.path[live[i]].append((t, q))
                    st[self.o_mc + (e * P + p) * P + q] += 1
                    break
                u -= rm[p]
        self.root = live[0]
        self.path[self.root] = []
        self._measure()


def draw(model, first, prow, rng, **kw):
    """mc_model.draw on the graph above: (weight, statistics vector)"""
    g = ARG(model, rng, **kw)
    st = g.stat
    mu, rho, E = model.mu, model.rho, model.E
    x = 0.0
    nxt = rng.expovariate(rho * g.ltree) if rho > 0 else INF
    w = 1.0
    segs = [(first, False, None)] + prow if first > 0 else prow
    for end, has_data, site in segs:
        while x < end:
            x1 = min(end, nxt)
            d = x1 - x
            if has_data:
                w *= fastexp(-mu * g.ltree * d)
            for e in range(E):
                st[g.o_ro + e] += g.lepoch[e] * d
            x = x1
            if x < end:
                g.recombine()
                nxt = x + rng.expovariate(rho * g.ltree)
        if site is not None:
            w *= g.site_likelihood(site)
    for e in range(E):                      # the last tree stays in force up to loci_length
        st[g.o_ro + e] += g.lepoch[e] * (model.L - x)
    return w, st


def accumulate(model_dict, rows, M, seed, **kw):
    """mc_model.accumulate with the draw above"""
    model = Model(model_dict)
    first, prow = prepare_rows(model, rows)
    rng = random.Random(seed)
    a = np.zeros(2)
    b1 = np.zeros(model.nstat); b2 = np.zeros(model.nstat); b3 = np.zeros(model.nstat)
    for _ in range(M):
        w, st = draw(model, first, prow, rng, **kw)
        s = np.array(st)
        a[0] += w; a[1] += w * w
        b1 += w * s; b2 += w * w * s; b3 += w * w * s * s
    return M, a, b1, b2, b3


def run(model_dict, rows, M, seed, **kw):
    return summarise(model_dict, [accumulate(model_dict, rows, M, seed, **kw)])


def simulate_sites(model_dict, seed):
    """mc_model.simulate_sites on the graph above: (positions, 0/1 patterns [sites, n])"""
    model = Model(model_dict)
    rng = random.Random(seed)
    nrng = np.random.default_rng(seed)
    g = ARG(model, rng)
    x, pos, pat = 0.0, [], []
    while x < model.L:
        x1 = min(model.L, x + rng.expovariate(model.rho * g.ltree))
        k = nrng.poisson(model.mu * g.ltree * (x1 - x))
        for pp in sorted(nrng.uniform(x, x1, k)):
            u = rng.random() * g.ltree
            for v in range(2 * model.n - 1):
                if v == g.root:
                    continue
                ln = g.height[g.parent[v]] - g.height[v]
                if u < ln:
                    break
                u -= ln
            row = [0] * model.n
            for leaf in g.leaves_below(v):
                row[leaf] = 1
            pos.append(float(pp)); pat.append(row)
        x = x1
        if x < model.L:
            g.recombine()
    return pos, pat
