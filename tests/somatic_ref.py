"""Two independent restatements of CanvasSomaticCaller's purity / ploidy grid search (ModelOverallCoverageAndPurity, SomaticCaller.cs:1870-2117, without the cluster term of
ModelDeviation), for the tests of canvas_somatic_model_fit.

  fit_scalar      (a) follows the C# statement by statement: plain loops, math.exp / math.log, numpy.float32(p) / numpy.float32(100) for the purity.
  fit_vectorised  (b) written differently: the distances of all models come from array operations, the ordered sums from np.add.accumulate along the segment axis (a
                  segment that does not belong to an accumulator adds +0.0, which leaves every sum's bits alone: no accumulator is ever -0.0), the selection from masks and
                  a stable argsort.  No np.sum, no math.fsum: they add in another order.

A case is a dict: coverage, maf (< 0: none), weight (float64), length (int32), cwf, genome_length, min_coverage, max_coverage, hard_limit, mmac, is_enrichment,
fixed_percent_purity, fixed_coverage (-1: none), params (overrides of DEFAULTS).  Both return the same dict (see _result)."""
import math

import numpy as np

DEFAULTS = dict(maximum_copy_number=8, deviation_index_cutoff=11, maximum_related_models=5, min_allowed_ploidy=0.5, max_allowed_ploidy=8.0, deviation_factor=1.75,
                cn2_weighting_factor=0.175, deviation_score_weighting_factor=0.375, diploid_distance_score_weighting_factor=0.125,
                heterogeneity_score_weighting_factor=0.202)
INFO_CLUSTER_TERM, INFO_INDEX_CUTOFF = 1, 2
VALID, SCORED = 1, 2
DBL_MAX = 1.7976931348623157e308


class NoModel(Exception):
    """no model passes the ploidy filter (UncallableDataException, :1934)"""


class NoScore(Exception):
    """no model scores above 0 (bestModel stays null, :2061)"""


def params_of(case):
    p = dict(DEFAULTS, **case.get("params", {}))
    for k in ("min_allowed_ploidy", "max_allowed_ploidy", "deviation_factor"):       # floats in SomaticCallerParameters
        p[k] = float(np.float32(p[k]))
    return p


def ploidies(max_cn):
    """InitializePloidies (:87-116): (CopyNumber, MajorChromosomeCount) in index order"""
    out = []
    for cn in range(max_cn + 1):
        major = cn
        while major * 2 >= cn:
            out.append((cn, major))
            major -= 1
    return out


def purity_of(percent, double_division=False):
    """model.Purity = percentPurity / 100f (:1918): a float quotient, widened"""
    return percent / 100.0 if double_division else float(np.float32(percent) / np.float32(100))


def grid_of(case):
    lo, hi = (case["fixed_coverage"],) * 2 if case.get("fixed_coverage", -1) >= 0 else (case["min_coverage"], case["max_coverage"])
    models = []
    for coverage in range(lo, hi + 1):
        lo_p = int(max(float(case["hard_limit"]), 100 * (1 - 2 * case["mmac"] / coverage) - 10))
        hi_p = 100
        if case.get("fixed_percent_purity", -1) >= 0:
            lo_p = hi_p = case["fixed_percent_purity"]
        for percent in range(lo_p, hi_p + 1):
            models.append((coverage, percent))
    return models


def info_of(case):
    n_maf = sum(1 for m in case["maf"] if m >= 0)
    return INFO_CLUSTER_TERM if (n_maf > 100 and len(case["maf"]) > 100 and not case.get("is_enrichment", False)) else 0


# ================================================================================================================ (a) scalar
class _Scalar:
    def __init__(self):
        self.log_factorial = [0.0, 0.0]

    def log_combinations(self, k, n):
        for i in range(max(2, len(self.log_factorial)), n + 1):
            self.log_factorial.append(math.log(i) + self.log_factorial[i - 1])
        return self.log_factorial[n] - self.log_factorial[k] - self.log_factorial[n - k]

    def binom_p(self, i, n, p):
        return math.exp(self.log_combinations(i, n) + i * math.log(p) + (n - i) * math.log(1 - p))

    def adjusted_maf(self, theoretical, coverage):
        if coverage < 1.0:
            return 0.0
        if theoretical == 0:
            return 0.0
        mean = theoretical / coverage
        mean_obs = 0.0
        for i in range(int(coverage) + 1):
            mean_obs += min(float(i), coverage - i) * self.binom_p(i, int(coverage), mean)
        return mean_obs / coverage

    def model_points(self, coverage, percent, max_cn, double_division=False):
        purity = purity_of(percent, double_division)
        tumor_haploid = coverage * purity / 2.0
        normal_haploid = coverage * (1.0 - purity) / 2.0
        pts = []
        for cn, major in ploidies(max_cn):
            cov = cn * tumor_haploid + 2 * normal_haploid
            theoretical = (cn - major) * tumor_haploid + normal_haploid
            pts.append(dict(cn=cn, major=major, coverage=cov, maf=self.adjusted_maf(theoretical, cov), weight=0.0, maf_weight=0.0, emp_cov=0.0, emp_maf=0.0))
        return pts


def distance(coverage, coverage2, maf, maf2, cwf):
    """GetModelDistance (:884-892)"""
    diff = (coverage - coverage2) * cwf
    d = diff * diff
    if maf < 0:
        return 2 * d
    diff = maf - maf2
    d += diff * diff
    return d


def _refine_diploid_maf(case, pts, max_cn):
    cov, maf, w, cwf = case["coverage"], case["maf"], case["weight"], case["cwf"]
    diploid_maf = [0.0] * (1 + max_cn // 2)
    diploid_w = [0.0] * (1 + max_cn // 2)
    dummy = 10000000.0
    for pt in pts:
        if pt["cn"] % 2 == 1 or pt["major"] * 2 != pt["cn"]:
            continue
        diploid_maf[pt["cn"] // 2] += dummy * pt["maf"]
        diploid_w[pt["cn"] // 2] += dummy
    for s in range(len(cov)):
        if maf[s] < 0:
            continue
        best_d, best = DBL_MAX, None
        for pt in pts:
            d = distance(float(cov[s]), pt["coverage"], float(maf[s]), pt["maf"], cwf)
            if d < best_d:
                best_d, best = d, pt
        if best["cn"] % 2 == 0 and best["major"] * 2 == best["cn"]:
            if maf[s] < 0.4:
                continue
            diploid_maf[best["cn"] // 2] += float(w[s]) * float(maf[s])
            diploid_w[best["cn"] // 2] += float(w[s])
    for pt in pts:
        if pt["cn"] % 2 == 1 or pt["major"] * 2 != pt["cn"]:
            continue
        pt["maf"] = diploid_maf[pt["cn"] // 2] / diploid_w[pt["cn"] // 2]


def model_deviation_scalar(case, pts, max_cn):
    """ModelDeviation (:1214-1379) without the cluster term, then DiploidModelDistance (:842-860)"""
    cov, maf, w, length, cwf = case["coverage"], case["maf"], case["weight"], case["length"], case["cwf"]
    _refine_diploid_maf(case, pts, max_cn)
    percent_cn = [0.0] * (max_cn + 1)
    cns, seg_point, seg_dist = [], [], []
    precision = total_weight = total_normal = 0.0
    for s in range(len(cov)):
        best_d, best, best_i = DBL_MAX, None, -1
        for i, pt in enumerate(pts):
            d = distance(float(cov[s]), pt["coverage"], float(maf[s]), pt["maf"], cwf)
            if d < best_d:
                best_d, best, best_i = d, pt, i
        best_d = math.sqrt(best_d)
        ws = float(w[s])
        precision += best_d * ws
        total_weight += ws
        percent_cn[best["cn"]] += ws
        if best["cn"] == 2 and best["major"] == 1:
            total_normal += ws
        best["weight"] += ws
        best["emp_cov"] += ws * float(cov[s])
        if maf[s] >= 0:
            best["emp_maf"] += ws * float(maf[s])
            best["maf_weight"] += ws
        cns.append(1 if (best["cn"] == 2 and best["major"] == 2) else best["cn"])
        seg_point.append(best_i)
        seg_dist.append(best_d)
    precision /= total_weight
    accuracy = 0.0
    for pt in pts:
        if pt["weight"] == 0:
            continue
        pt["emp_cov"] /= pt["weight"]
        if pt["maf_weight"] > 0:
            pt["emp_maf"] /= pt["maf_weight"]
        accuracy += math.sqrt(distance(pt["coverage"], pt["emp_cov"], pt["maf"], pt["emp_maf"], cwf)) * pt["weight"]
    accuracy /= total_weight
    for i in range(max_cn + 1):
        percent_cn[i] /= total_weight
    ploidy = 0.0
    for i in range(max_cn + 1):
        ploidy += i * percent_cn[i]
    deviation = precision * 0.5 + 0.5 * accuracy
    # DiploidModelDistance
    events, baseline, amplification = 0.0, 2, 0.0
    for cn in range(3, max_cn):
        amplification += percent_cn[cn]
    if amplification > 0.8:
        baseline = 4
        events += 1
    for s in range(len(cns)):
        events += int(np.int32(abs(cns[s] - baseline)) * np.int32(length[s])) / float(case["genome_length"])
    return dict(deviation=deviation, precision_deviation=precision, accuracy_deviation=accuracy, ploidy=ploidy, percent_normal=total_normal / total_weight,
                percent_cn=percent_cn, diploid_distance=1.0 / max(0.001, events), cns=cns, seg_point=seg_point, seg_distance=seg_dist, points=pts)


def fit_scalar(case, double_division=False):
    p = params_of(case)
    max_cn = p["maximum_copy_number"]
    grid = grid_of(case)
    sc = _Scalar()
    every = [model_deviation_scalar(case, sc.model_points(c, pc, max_cn, double_division), max_cn) for c, pc in grid]
    for m, (c, pc) in zip(every, grid):
        m["purity"] = purity_of(pc, double_division)
    # ---- :1921-1937
    best_deviation = DBL_MAX
    all_models = []
    for i, m in enumerate(every):
        ok = m["ploidy"] < p["max_allowed_ploidy"] and m["ploidy"] > p["min_allowed_ploidy"]
        if m["deviation"] < best_deviation and ok:
            best_deviation = m["deviation"]
        if ok:
            all_models.append(i)
    flags = [0] * len(every)
    scores_by_model = [0.0] * len(every)
    for i in all_models:
        flags[i] = VALID
    res = _result(case, grid, every, flags, scores_by_model, info_of(case), len(all_models))
    if not all_models:
        raise NoModel(res)
    # ---- :1947-1976
    worst = best_deviation * p["deviation_factor"]
    counter, deviations = 0, []
    for i in all_models:
        if every[i]["deviation"] < worst:
            counter += 1
        deviations.append(every[i]["deviation"])
    deviations.sort()
    res["counter"] = counter
    if counter < p["deviation_index_cutoff"]:
        worst = deviations[min(p["deviation_index_cutoff"], len(deviations) - 1)]
        res["info"] |= INFO_INDEX_CUTOFF
    best_cn2 = best_dd = 0.0
    for i in all_models:
        m = every[i]
        if m["deviation"] > worst:
            continue
        if m["percent_cn"][2] > best_cn2:
            best_cn2 = m["percent_cn"][2]
        if m["diploid_distance"] > best_dd:
            best_dd = m["diploid_distance"]
    # ---- :1979-2056
    best_models, scores, best, best_score = [], [], None, 0.0
    hard = case["hard_limit"] / 100.0
    for i in all_models:
        m = every[i]
        if m["deviation"] > worst:
            continue
        low_purity = 1.5 / ((1.5 - 0.5) / (1.0 - hard) * (m["purity"] - hard) + 1.0)
        cn2_score = low_purity * p["cn2_weighting_factor"] * (m["percent_cn"][2] / max(0.01, best_cn2) - 1)
        dev_score = 0.0
        if worst > best_deviation:
            dev_score = p["deviation_score_weighting_factor"] * (worst - m["deviation"]) / (worst - best_deviation)
        dd_score = p["diploid_distance_score_weighting_factor"] * m["diploid_distance"] / max(0.01, best_dd)
        het_score = p["heterogeneity_score_weighting_factor"] * 0.0
        score = cn2_score + dev_score + dd_score + het_score
        scores.append(score)
        best_models.append(i)
        scores_by_model[i] = score
        flags[i] |= SCORED
        if score > best_score:
            best, best_score = i, score
    res.update(nscored=len(best_models), best_deviation=best_deviation, worst_allowed_deviation=worst)
    if best is None:
        raise NoScore(res)
    # ---- :2083-2094
    order = sorted(range(len(scores)), key=lambda k: -scores[k])        # OrderBy is stable, and so is sorted()
    inter = 0.0
    for k in range(1, min(len(order), p["maximum_related_models"])):
        a, b = every[best_models[order[0]]]["cns"], every[best_models[order[k]]]["cns"]
        g = 0.0
        for s in range(len(a)):
            g += int(np.int32(abs(a[s] - b[s])) * np.int32(case["length"][s])) / float(case["genome_length"])
        inter += g
    inter /= float(p["maximum_related_models"])
    m = every[best]
    res.update(model=best, coverage=grid[best][0], percent_purity=grid[best][1], purity=m["purity"], score=best_score, inter_model_distance=inter,
               seg_point=np.array(m["seg_point"], np.int32), seg_distance=np.array(m["seg_distance"], np.float64), ncandidates=len(order),
               **{k: m[k] for k in ("deviation", "precision_deviation", "accuracy_deviation", "ploidy", "percent_normal", "diploid_distance")})
    res["percent_cn"] = np.array(m["percent_cn"], np.float64)
    return res


def _result(case, grid, every, flags, scores, info, nvalid):
    col = lambda k: np.array([m[k] for m in every], np.float64)
    return dict(nmodels=len(grid), nvalid=nvalid, nscored=0, info=info, model=-1,
                models=dict(coverage=np.array([g[0] for g in grid], np.int32), percent_purity=np.array([g[1] for g in grid], np.int32), deviation=col("deviation"),
                            precision_deviation=col("precision_deviation"), accuracy_deviation=col("accuracy_deviation"), ploidy=col("ploidy"), percent_normal=col("percent_normal"),
                            percent_cn=np.array([m["percent_cn"] for m in every], np.float64), diploid_distance=col("diploid_distance"), flags=flags, score=scores),
                points=[[(pt["coverage"], pt["maf"]) for pt in m["points"]] for m in every] if every and "points" in every[0] else None)


# ================================================================================================================ (b) vectorised
def table_vectorised(grid, max_cn, double_division=False):
    """coverage and MAF of every model's points, (M, P) each: the binomial terms of one point are built as lists over i, and only their running sum is a loop"""
    pl = np.array(ploidies(max_cn), np.int64)
    cn, minor = pl[:, 0].astype(np.float64), (pl[:, 0] - pl[:, 1]).astype(np.float64)
    cov = np.array([g[0] for g in grid], np.float64)
    pur = np.array([purity_of(g[1], double_division) for g in grid], np.float64)
    th, nh = cov * pur / 2.0, cov * (1.0 - pur) / 2.0
    pc = cn[None, :] * th[:, None] + 2 * nh[:, None]
    ma = minor[None, :] * th[:, None] + nh[:, None]
    nmax = int(pc.max()) + 1
    lf = [0.0, 0.0]
    for i in range(2, nmax + 1):
        lf.append(math.log(i) + lf[-1])
    pm = np.zeros_like(pc)
    cache = {}
    for idx in np.ndindex(pc.shape):
        c, t = float(pc[idx]), float(ma[idx])
        if c < 1.0 or t == 0:
            continue
        if (c, t) not in cache:
            n, mean = int(c), t / c
            lp, lq = math.log(mean), math.log(1 - mean)
            terms = [min(float(i), c - i) * math.exp(lf[n] - lf[i] - lf[n - i] + i * lp + (n - i) * lq) for i in range(n + 1)]
            cache[(c, t)] = float(np.add.accumulate(np.array([0.0] + terms))[-1]) / c
        pm[idx] = cache[(c, t)]
    return pc, pm


def _ordered(values, seed=None):
    """sum along the last axis in index order (np.add.accumulate is sequential), starting from `seed` (0.0 unless given)"""
    values = np.asarray(values, np.float64)
    seed = np.zeros(values.shape[:-1]) if seed is None else np.asarray(seed, np.float64)
    return np.add.accumulate(np.concatenate([seed[..., None], values], axis=-1), axis=-1)[..., -1]


def _nearest(case, pc, pm):
    """squared distance to the nearest point and its index for every (model, segment); np.argmin keeps the first minimum"""
    cov, maf, cwf = case["coverage"], case["maf"], case["cwf"]
    dc = (cov[None, :, None] - pc[:, None, :]) * cwf
    dc2 = dc * dc
    dm = maf[None, :, None] - pm[:, None, :]
    d = np.where((maf < 0)[None, :, None], 2 * dc2, dc2 + dm * dm)
    idx = np.argmin(d, axis=2)
    return np.take_along_axis(d, idx[:, :, None], axis=2)[:, :, 0], idx


def deviations_vectorised(case, pc, pm, max_cn):
    cov, maf, w, length, cwf = case["coverage"], case["maf"], case["weight"], case["length"], case["cwf"]
    pl = np.array(ploidies(max_cn), np.int64)
    pcn, pmajor = pl[:, 0], pl[:, 1]
    M, P = pc.shape
    even = np.nonzero((pcn % 2 == 0) & (pmajor * 2 == pcn))[0]
    pm = pm.copy()
    # RefineDiploidMAF
    _, idx = _nearest(case, pc, pm)
    use = (maf >= 0) & ~(maf < 0.4)
    for e in even:
        member = (idx == e) & use[None, :]
        num = _ordered(np.where(member, (w * maf)[None, :], 0.0), 10000000.0 * pm[:, e])
        den = _ordered(np.where(member, w[None, :], 0.0), np.full(M, 10000000.0))
        pm[:, e] = num / den
    # the clustering loop
    d2, idx = _nearest(case, pc, pm)
    dist = np.sqrt(d2)
    total_weight = _ordered(w)
    precision = _ordered(dist * w[None, :]) / total_weight
    onehot = idx[:, :, None] == np.arange(P)[None, None, :]                                   # (M, S, P)
    per_point = lambda v: _ordered(np.where(onehot, v[None, :, None], 0.0).transpose(0, 2, 1))      # -> (M, P)
    has = maf >= 0
    weight, emp_cov = per_point(w), per_point(w * cov)
    emp_maf, maf_weight = per_point(np.where(has, w * maf, 0.0)), per_point(np.where(has, w, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        emp_cov = emp_cov / weight
        emp_maf = np.where(maf_weight > 0, emp_maf / maf_weight, emp_maf)
        dc = (pc - emp_cov) * cwf
        dm = pm - emp_maf
        pdist = np.sqrt(dc * dc + dm * dm) * weight
    # the reference skips points of weight 0; the others are added in point order
    accuracy = np.zeros(M)
    for p in range(P):
        accuracy = np.where(weight[:, p] == 0, accuracy, accuracy + pdist[:, p])
    accuracy = accuracy / total_weight
    best_cn = pcn[idx]
    percent_cn = np.stack([_ordered(np.where(best_cn == c, w[None, :], 0.0)) for c in range(max_cn + 1)], axis=1) / total_weight
    ploidy = _ordered(np.arange(max_cn + 1)[None, :] * percent_cn, np.zeros(M))
    normal = _ordered(np.where((best_cn == 2) & (pmajor[idx] == 1), w[None, :], 0.0)) / total_weight
    cns = np.where((best_cn == 2) & (pmajor[idx] == 2), 1, best_cn).astype(np.int32)
    amplified = _ordered(percent_cn[:, 3:max_cn], np.zeros(M)) > 0.8
    baseline = np.where(amplified, 4, 2).astype(np.int32)
    terms = (np.abs(cns - baseline[:, None]).astype(np.int32) * length[None, :].astype(np.int32)) / float(case["genome_length"])
    events = _ordered(terms, np.where(amplified, 1.0, 0.0))
    return dict(deviation=precision * 0.5 + 0.5 * accuracy, precision_deviation=precision, accuracy_deviation=accuracy, ploidy=ploidy, percent_normal=normal,
                percent_cn=percent_cn, diploid_distance=1.0 / np.maximum(0.001, events), cns=cns, seg_point=idx.astype(np.int32), seg_distance=dist)


def fit_vectorised(case, double_division=False, chunk=64):
    p = params_of(case)
    max_cn = p["maximum_copy_number"]
    grid = grid_of(case)
    M = len(grid)
    case = dict(case, coverage=np.asarray(case["coverage"], np.float64), maf=np.asarray(case["maf"], np.float64), weight=np.asarray(case["weight"], np.float64),
                length=np.asarray(case["length"], np.int32))
    pc, pm = table_vectorised(grid, max_cn, double_division)
    parts = [deviations_vectorised(case, pc[i:i + chunk], pm[i:i + chunk], max_cn) for i in range(0, M, chunk)]
    col = {k: np.concatenate([q[k] for q in parts], axis=0) for k in parts[0]}
    purity = np.array([purity_of(g[1], double_division) for g in grid])
    valid = (col["ploidy"] < p["max_allowed_ploidy"]) & (col["ploidy"] > p["min_allowed_ploidy"])
    flags = np.where(valid, VALID, 0)
    score = np.zeros(M)
    res = dict(nmodels=M, nvalid=int(np.count_nonzero(valid)), nscored=0, info=info_of(case), model=-1, points=None,
               models=dict(coverage=np.array([g[0] for g in grid], np.int32), percent_purity=np.array([g[1] for g in grid], np.int32), flags=flags, score=score,
                           **{k: col[k] for k in ("deviation", "precision_deviation", "accuracy_deviation", "ploidy", "percent_normal", "percent_cn", "diploid_distance")}))
    if not valid.any():
        raise NoModel(res)
    dev = col["deviation"]
    best_deviation = dev[valid].min()
    worst = best_deviation * p["deviation_factor"]
    counter = int(np.count_nonzero(dev[valid] < worst))
    res["counter"] = counter
    if counter < p["deviation_index_cutoff"]:
        worst = np.sort(dev[valid])[min(p["deviation_index_cutoff"], res["nvalid"] - 1)]
        res["info"] |= INFO_INDEX_CUTOFF
    scored = valid & ~(dev > worst)
    best_cn2 = max(0.0, col["percent_cn"][scored, 2].max()) if scored.any() else 0.0
    best_dd = max(0.0, col["diploid_distance"][scored].max()) if scored.any() else 0.0
    hard = case["hard_limit"] / 100.0
    low_purity = 1.5 / (1.0 / (1.0 - hard) * (purity - hard) + 1.0)
    total = low_purity * p["cn2_weighting_factor"] * (col["percent_cn"][:, 2] / max(0.01, best_cn2) - 1)
    if worst > best_deviation:
        total = total + p["deviation_score_weighting_factor"] * (worst - dev) / (worst - best_deviation)
    else:
        total = total + 0.0
    total = total + p["diploid_distance_score_weighting_factor"] * col["diploid_distance"] / max(0.01, best_dd)
    total = total + p["heterogeneity_score_weighting_factor"] * 0.0
    score[scored] = total[scored]
    flags[scored] |= SCORED
    res.update(nscored=int(np.count_nonzero(scored)), best_deviation=float(best_deviation), worst_allowed_deviation=float(worst))
    cand = np.nonzero(scored)[0]
    if not (total[cand] > 0).any():
        raise NoScore(res)
    best = int(cand[np.argmax(total[cand])])                         # the first of the highest
    order = cand[np.argsort(-total[cand], kind="stable")][:p["maximum_related_models"]]
    assert order[0] == best
    diffs = (np.abs(col["cns"][order[1:]] - col["cns"][order[0]][None, :]).astype(np.int32) * case["length"][None, :]) / float(case["genome_length"])
    inter = _ordered(_ordered(diffs, np.zeros(len(order) - 1)), np.zeros(())) / float(p["maximum_related_models"]) if len(order) > 1 else 0.0 / float(p["maximum_related_models"])
    res.update(model=best, coverage=grid[best][0], percent_purity=grid[best][1], purity=float(purity[best]), score=float(total[best]), inter_model_distance=float(inter),
               seg_point=col["seg_point"][best], seg_distance=col["seg_distance"][best], ncandidates=len(cand), percent_cn=col["percent_cn"][best],
               **{k: float(col[k][best]) for k in ("deviation", "precision_deviation", "accuracy_deviation", "ploidy", "percent_normal", "diploid_distance")})
    return res
