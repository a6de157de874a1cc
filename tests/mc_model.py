"""The filter's model for any number of samples and populations, stated once more in plain Python: a prior sampler of
SMC' ancestral recombination graphs, the emission the filter weights by, and a brute-force Monte Carlo estimate of
p(data | model) and of the posterior expectation of every sufficient statistic of the E-step.

TEST INFRASTRUCTURE (numpy and the standard library only).  Nothing here comes from the reference, from oracle/ or from
smcsmc_amd: it is an independent statement of the *model*, written from DESIGN.md (sections 3a, 4 and 6), the way
tests/exact_hmm2.py is one for two samples.  A particle filter's estimate of the normalising constant is unbiased at
any number of particles, with or without resampling, focused sampling, a guide or the look-ahead, so
E_seeds[exp(logl)] of the oracle and of the device must equal the number computed here, and their (fully smoothed)
counts must equal the weighted means computed here.  tests/golden/make_mc_model.py runs this once per case and stores
the numbers in tests/golden/mc_model.json.

Model (times in generations, positions in bp; the dictionary of tests/cases.py::make_model / make_structured):
  * E epochs starting at change_times[e]; P populations of size pop_sizes[e, p]; lineages coalesce pairwise only within
    a population, at rate 1 / (2 N_p(t)) per pair; every lineage migrates from a to b at rate mig_rates[e, a, b];
    single_mig[e, a, b] = 1 moves every lineage of a to b at the start of epoch e (a join; not a migration event);
    sample i starts at time 0 in sample_pops[i].
  * The tree at position 0 is a draw of this structured coalescent.  Along the sequence recombinations arrive at rate
    recombination_rate x (length of the local tree) per bp.  The cut is uniform on the tree's length.  The part of the
    cut branch above the cut (the stub) stays in place; a floating lineage starts at the cut, in the population the
    branch occupies at that height, migrates like any lineage and joins each lineage of its own population that is
    present at the time -- the branches of the old tree, the stub of its own branch included (SMC': the tree is then
    unchanged, the branch takes the new path up to the joining point) -- at rate 1 / (2 N_p).  Above the old root the
    root's lineage continues as one lineage that keeps migrating, and the two race.  Then the rest of the stub is
    dropped.  Every branch carries its population path as a short list of (time, population).

Target (what the filter multiplies into a particle's weight; DESIGN.md section 6, item 3, for any n):
  * rows as Segments.pack hands them over: [start, start + length) in bp from 0, clipped at loci_length;
  * along a row in which every sample has data: fastexp(-mu x Ltree x d) for every stretch of d bases between two
    consecutive recombinations or row ends, Ltree the length of the local tree (fastexp: the Pade form of
    tests/cases.py::fastexp, part of the target's definition); along a row in which every sample is missing: nothing;
  * a row of state 0 has a site at its end: the pruning likelihood of the tree in force there, two alleles, root prior
    1/2, 1/2, no change along a branch of length b with probability fastexp(-mu b), the other allele otherwise; a missing
    leaf has likelihood 1 for both alleles (so an all-missing row contributes 1);
  * unphased pairs: a site whose row has the marks (2, 2) at samples (2k, 2k + 1) for k of its pairs weighs the arithmetic
    mean, over the 2^k assignments (0, 1) / (1, 0) of those pairs, of the pruning likelihood above; a mark anywhere else (one
    sample of a pair, the unpaired last sample of an odd n) is not data and is refused;
  * model key dephase: every pair (2k, 2k + 1) whose two alleles are {0, 1} counts as marked, whatever its order;
  * model key ancestral_aware: the root prior is 1 on allele 0 and 0 on allele 1;
  * rows in which only some samples are missing are still not stated here (the tracked-branch rule of such rows is not part
    of this statement): run() refuses them.
  p(data | model) is the prior expectation of the product of these factors.

Sufficient statistics, as functionals of the ancestral recombination graph (all recorded: lags beyond the sequence):
  * rec_opp[e]: (length of the local tree inside epoch e) x (bases it is in force), from position 0 to loci_length -- the
    rows of a packed file end one base earlier (its coordinates start at the file's base 1), the filter extends its
    particles to the end of the last row and closes the opportunity of the tree it then has at loci_length;
    rec_count[e]: recombinations whose cut height lies in e (those that re-join their own stub included);
  * coal_opp[e, p]: for every recombination, the number of lineages the floating lineage can join in its population
    (branches of the old tree in p, its own stub, above the old root the root's lineage), integrated over the time it
    floats in (e, p); coal_count[e, p]: where it joins (its own stub included);
  * mig_opp[e, p]: the time the floating lineage spends in (e, p), plus the time the root's lineage spends there while
    the floating lineage is above the old root; mig_count[e, a, b]: migrations of either in that time (joins excluded);
  * the tree at position 0 is counted once, at position 0, as if its samples had been added one at a time to the tree of
    those before them: given the tree that is coal_opp[e, p] += (pairs of lineages in p) dt, one coal_count per node,
    mig_opp[e, p] += (lineages in p) dt and one mig_count per migration on it (for two samples and one population:
    |[0, s] n e| and one event, lines 18-22 of tests/exact_hmm2.py).

run(model, rows, M, seed) draws M graphs from the prior and returns log of the mean weight, its relative standard error
and the self-normalised means of the statistics with delta-method standard errors.  Two switches exist for the
sensitivity table of the profiles page only: smc_prime=False (no re-joining of the own stub) and float_start="sample"
(the floating lineage starts in the population of the lowest sample below the cut, moved by the joins passed but not by
the migrations on the branch).
"""
import bisect
import math
import random

import numpy as np

INF = float("inf")


def fastexp(x):
    """tests/cases.py::fastexp for one number (test_mc_model_cpu.py holds the two to each other)"""
    xx = x * x
    if xx < 0.516167859:
        return 1 + 2 * x / (2 - x + xx / (6 + xx * 0.1))
    return math.exp(x)


class Model:
    def __init__(self, m):
        self.T = [float(t) for t in m["change_times"]]
        E = self.E = len(self.T)
        P = self.P = int(m.get("n_pops", 1))
        self.n = int(m["nsam"])
        self.N = np.asarray(m["pop_sizes"], float).reshape(E, P).tolist()
        mr = np.asarray(m["mig_rates"], float).reshape(E, P, P) if m.get("mig_rates") is not None else np.zeros((E, P, P))
        self.mig = mr.tolist()
        self.mtot = [[sum(mr[e, a, b] for b in range(P) if b != a) for a in range(P)] for e in range(E)]
        sm = np.asarray(m["single_mig"], float).reshape(E, P, P) if m.get("single_mig") is not None else np.zeros((E, P, P))
        self.jmap = [[a for a in range(P)] for _ in range(E)]
        for e in range(E):
            for a in range(P):
                for b in range(P):
                    if sm[e, a, b] != 0:
                        assert sm[e, a, b] == 1.0 and a != b, "deterministic joins only"
                        self.jmap[e][a] = b
        self.spop = [int(q) for q in m.get("sample_pops", [0] * self.n)]
        self.mu = float(m["mutation_rate"])
        self.rho = float(m["recombination_rate"])
        self.L = float(m["loci_length"])
        self.dephase = bool(m.get("dephase", False))
        self.root_prior = (1.0, 0.0) if m.get("ancestral_aware", False) else (0.5, 0.5)
        self.nstat = 2 * E + 3 * E * P + E * P * P

    def epoch_of(self, t):
        return bisect.bisect_right(self.T, t) - 1

    def epoch_end(self, e):
        return self.T[e + 1] if e + 1 < self.E else INF

    def unpack(self, v):
        E, P = self.E, self.P
        v = np.asarray(v)
        o = [0]

        def take(*shape):
            k = int(np.prod(shape))
            out = v[o[0]:o[0] + k].reshape(shape)
            o[0] += k
            return out
        return dict(rec_count=take(E), rec_opp=take(E), coal_count=take(E, P), coal_opp=take(E, P),
                    mig_count=take(E, P, P), mig_opp=take(E, P))


class ARG:
    """One graph drawn along the sequence.  Nodes 0..n-1 are the samples, n..2n-2 the coalescences; parent[v] < 0 for the
    root; pop0[v] the population at the bottom of the branch above v, path[v] its later (time, population) changes."""

    def __init__(self, model, rng, smc_prime=True, float_start="branch"):
        self.m = model
        self.rng = rng
        self.smc_prime = smc_prime
        self.float_start = float_start
        m = model
        E, P = m.E, m.P
        # offsets into the flat statistics vector
        self.o_rc, self.o_ro = 0, E
        self.o_cc, self.o_co = 2 * E, 2 * E + E * P
        self.o_mc = 2 * E + 2 * E * P
        self.o_mo = self.o_mc + E * P * P
        self.stat = [0.0] * m.nstat
        self._initial_tree()

    # ---- the tree at position 0: the structured coalescent, all lineages at once
    def _initial_tree(self):
        m, rng, st = self.m, self.rng, self.stat
        n, P = m.n, m.P
        self.height = [0.0] * (2 * n - 1)
        self.parent = [-1] * (2 * n - 1)
        self.child = [None] * (2 * n - 1)
        self.pop0 = list(m.spop) + [0] * (n - 1)
        self.path = [[] for _ in range(2 * n - 1)]
        live = list(range(n))
        cur = list(m.spop)                       # current population of every live lineage
        t, e, nxt = 0.0, 0, n
        while len(live) > 1:
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

    def _mig_target(self, e, p):
        m = self.m
        u = self.rng.random() * m.mtot[e][p]
        last = -1
        for q in range(m.P):
            r = m.mig[e][p][q]
            if q == p or r == 0.0:
                continue
            last = q
            if u < r:
                return q
            u -= r
        return last

    def _measure(self):
        """tree length, and its part inside every epoch"""
        m = self.m
        le = [0.0] * m.E
        tot = 0.0
        for v in range(2 * m.n - 1):
            if v == self.root:
                continue
            a, b = self.height[v], self.height[self.parent[v]]
            tot += b - a
            for e in range(m.epoch_of(a), m.E):
                lo, hi = max(a, m.T[e]), min(b, m.epoch_end(e))
                if hi > lo:
                    le[e] += hi - lo
                if m.epoch_end(e) >= b:
                    break
        self.ltree, self.lepoch = tot, le

    def pop_at(self, v, t):
        q = self.pop0[v]
        for tm, qq in self.path[v]:
            if tm <= t:
                q = qq
            else:
                break
        return q

    def lowest_sample(self, v):
        while v >= self.m.n:
            v = min(self.lowest_sample(c) for c in self.child[v])
        return v

    # ---- one recombination at the current tree
    def recombine(self):
        m, rng, st = self.m, self.rng, self.stat
        n, P = m.n, m.P
        nodes = range(2 * n - 1)
        # the cut: uniform on the tree's length
        u = rng.random() * self.ltree
        b = -1
        for v in nodes:
            if v == self.root:
                continue
            ln = self.height[self.parent[v]] - self.height[v]
            b = v
            if u < ln:
                break
            u -= ln
        h = self.height[b] + min(u, self.height[self.parent[b]] - self.height[b])
        st[self.o_rc + m.epoch_of(h)] += 1
        p_old = self.parent[b]
        Sp = self.height[p_old]
        Hr = self.height[self.root]
        if self.float_start == "branch":
            pf = self.pop_at(b, h)
        else:                                   # (sensitivity table only) the sample's population, moved by the joins alone
            pf = m.spop[self.lowest_sample(b)]
            for ee in range(1, m.epoch_of(h) + 1):
                pf = m.jmap[ee][pf]
        pr = self.pop0[self.root]
        # where the configuration of the old tree changes above the cut
        marks = set(self.height[v] for v in range(n, 2 * n - 1) if self.height[v] > h)
        for v in nodes:
            for tm, _ in self.path[v]:
                if tm > h:
                    marks.add(tm)
        for tb in m.T:
            if tb > h:
                marks.add(tb)
        marks = sorted(marks) + [INF]
        picked, rpicked = [], []
        t, e = h, m.epoch_of(h)
        target = None
        for t_next in marks:
            while True:
                root_active = t >= Hr
                cands = []
                for v in nodes:
                    if v == self.root:
                        continue
                    if self.height[v] <= t < self.height[self.parent[v]] and self.pop_at(v, t) == pf:
                        if v == b and not self.smc_prime:
                            continue
                        cands.append(v)
                if root_active and pr == pf:
                    cands.append(-1)
                w = len(cands)
                rc = w / (2.0 * m.N[e][pf])
                rmf = m.mtot[e][pf]
                rmr = m.mtot[e][pr] if root_active else 0.0
                lam = rc + rmf + rmr
                dt = rng.expovariate(lam) if lam > 0 else INF
                hit = t + dt < t_next
                t1 = t + dt if hit else t_next
                assert t1 < INF, "the floating lineage can never join"
                st[self.o_co + e * P + pf] += w * (t1 - t)
                st[self.o_mo + e * P + pf] += t1 - t
                if root_active:
                    st[self.o_mo + e * P + pr] += t1 - t
                t = t1
                if not hit:
                    break
                x = rng.random() * lam
                if x < rc:
                    st[self.o_cc + e * P + pf] += 1
                    target = cands[min(int(x / rc * w), w - 1)]
                    break
                if x < rc + rmf:
                    q = self._mig_target(e, pf)
                    st[self.o_mc + (e * P + pf) * P + q] += 1
                    picked.append((t, q))
                    pf = q
                else:
                    q = self._mig_target(e, pr)
                    st[self.o_mc + (e * P + pr) * P + q] += 1
                    rpicked.append((t, q))
                    pr = q
            if target is not None:
                break
            if e + 1 < m.E and t == m.T[e + 1]:
                e += 1
                q = m.jmap[e][pf]
                if q != pf:
                    picked.append((t, q)); pf = q
                if t >= Hr:
                    q = m.jmap[e][pr]
                    if q != pr:
                        rpicked.append((t, q)); pr = q
        tc = t
        below = [ev for ev in self.path[b] if ev[0] <= h]
        if target == b:
            # back into its own stub: same tree, the branch takes the new path up to tc
            self.path[b] = below + picked + [ev for ev in self.path[b] if ev[0] > tc]
            return
        # prune: the sibling's branch continues through the removed parent
        sib = [c for c in self.child[p_old] if c != b][0]
        g = self.parent[p_old]
        self.path[sib] = self.path[sib] + self.path[p_old]
        self.parent[sib] = g
        if g >= 0:
            self.child[g] = [sib if c == p_old else c for c in self.child[g]]
        else:
            self.root = sib
        self.path[self.root] = self.path[self.root] + rpicked
        if target == p_old:
            target = sib
        if target == -1:
            target = self.root
        # regraft: p_old becomes the new node on the target's branch
        gp = self.parent[target] if target != self.root else -1
        self.height[p_old] = tc
        self.pop0[p_old] = pf
        self.child[p_old] = [b, target]
        self.parent[p_old] = gp
        if gp >= 0:
            self.child[gp] = [p_old if c == target else c for c in self.child[gp]]
            self.path[p_old] = [ev for ev in self.path[target] if ev[0] > tc]
        else:
            self.root = p_old
            self.path[p_old] = []
        self.path[target] = [ev for ev in self.path[target] if ev[0] <= tc]
        self.parent[target] = p_old
        self.parent[b] = p_old
        self.path[b] = below + picked
        self.path[self.root] = []               # nothing is kept above the root of the local tree
        self._measure()

    # ---- emission
    def site_likelihood(self, alleles):
        """the weight of a site: the pruning likelihood, or its mean over the phasings of the marked pairs"""
        m = self.m
        pairs = [i for i in range(0, m.n - 1, 2)
                 if alleles[i] == 2 or (m.dephase and alleles[i] + alleles[i + 1] == 1 and alleles[i] * alleles[i + 1] == 0)]
        if not pairs:
            return self.pruning_likelihood(alleles)
        a = list(alleles)
        total = 0.0
        for bits in range(1 << len(pairs)):
            for k, i in enumerate(pairs):
                a[i], a[i + 1] = (1, 0) if (bits >> k) & 1 else (0, 1)
            total += self.pruning_likelihood(a)
        return total / (1 << len(pairs))

    def pruning_likelihood(self, alleles):
        m = self.m
        mu = m.mu

        def up(v):
            if v < m.n:
                a = alleles[v]
                return (1.0 if a != 1 else 0.0), (1.0 if a != 0 else 0.0)
            l0 = l1 = 1.0
            for c in self.child[v]:
                c0, c1 = up(c)
                p = fastexp(-(self.height[v] - self.height[c]) * mu)
                l0 *= c0 * p + c1 * (1 - p)
                l1 *= c1 * p + c0 * (1 - p)
            return l0, l1
        r0, r1 = up(self.root)
        return m.root_prior[0] * r0 + m.root_prior[1] * r1

    def leaves_below(self, v):
        if v < self.m.n:
            return [v]
        return [x for c in self.child[v] for x in self.leaves_below(c)]


def prepare_rows(model, rows):
    """[(end, has_data, alleles of the site at the end or None)] from packed rows, and the first position with data"""
    start = np.asarray(rows["start"], float)
    length = np.asarray(rows["length"], float)
    al = np.asarray(rows["alleles"]).reshape(len(start), -1)
    assert al.shape[1] == model.n
    out = []
    for s in range(len(start)):
        miss = int((al[s] < 0).sum())
        if miss not in (0, model.n):
            raise ValueError("rows with some samples missing are not stated in this model")
        marked = al[s] == 2
        if (marked[0:model.n - 1:2] != marked[1:model.n:2]).any() or (model.n % 2 == 1 and marked[-1]):
            raise ValueError("an unphased mark stands for a pair (2k, 2k + 1): a lone one is not data")
        assert s == 0 or start[s] == start[s - 1] + length[s - 1], "rows must be contiguous"
        end = min(start[s] + length[s], model.L)
        site = [int(a) for a in al[s]] if int(rows["state"][s]) == 0 and miss == 0 else None
        out.append((end, miss == 0, site))
    return float(start[0]), out


def draw(model, first, prow, rng, **kw):
    """one graph from the prior along the rows: (weight, statistics vector)"""
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
    """additive sums over M draws: [sum w, sum w^2], sum w s, sum w^2 s, sum w^2 s^2"""
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


def summarise(model_dict, parts):
    """parts: results of accumulate() -> dict(logp, logp_rse, cv, M, stats{name: array}, se{name: array})"""
    model = Model(model_dict)
    M = sum(p[0] for p in parts)
    a = sum(p[1] for p in parts); b1 = sum(p[2] for p in parts); b2 = sum(p[3] for p in parts); b3 = sum(p[4] for p in parts)
    mean = a[0] / M
    cv2 = M * a[1] / (a[0] * a[0]) - 1.0
    s = b1 / a[0]
    var = (b3 - 2 * s * b2 + s * s * a[1]) / (a[0] * a[0])          # delta method: sum w^2 (s_i - s)^2 / (sum w)^2
    return dict(M=int(M), logp=float(math.log(mean)), logp_rse=float(math.sqrt(max(cv2, 0.0) / M)), cv=float(math.sqrt(max(cv2, 0.0))),
                stats=model.unpack(s), se=model.unpack(np.sqrt(np.maximum(var, 0.0))))


def run(model_dict, rows, M, seed, **kw):
    return summarise(model_dict, [accumulate(model_dict, rows, M, seed, **kw)])


def tree_at(model, rng, position, **kw):
    """the graph of a prior draw at `position` bases from the start, with the tree at position 0 as (root height, length)"""
    g = ARG(model, rng, **kw)
    first = (g.height[g.root], g.ltree)
    x = rng.expovariate(model.rho * g.ltree)
    while x < position:
        g.recombine()
        x += rng.expovariate(model.rho * g.ltree)
    return g, first


def no_rows(model_dict, length):
    """one all-missing row without a site: the prior along `length` bases"""
    n = int(model_dict["nsam"])
    return dict(start=[0.0], length=[float(length)], state=[1], alleles=[[-1] * n])


def simulate_sites(model_dict, seed):
    """Data from the model itself: the graph run forward with infinite-sites mutations at rate mu per bp and generation.
    Returns (positions, 0/1 patterns [sites, n])."""
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
