"""Evaluation of an attribute edit: the scores of the sweeps of transeditor_amd.edit.edit_sweep laid out as the reference's
our_interfaceGAN/editing_evaluate.py:164-196 lays them out, and the dependency figure of our_interfaceGAN/calculate_score.py:45-71 (how
much an attribute of interest moves while the edited attribute changes); and the same for identity: the feature vectors of the sweeps
in the layout of our_interfaceGAN/editing_evaluate_id.py:162-195 and the identity-drift figure of our_interfaceGAN/calculate_score_id.py:
58-90.  Host code on small arrays; the scorers and the embedding network run on the device.

    sweeps = edit.edit_sweep(G, z_plus, p_plus, zb, pb, z_distance=30, p_distance=30, steps=6, batch=16)
    scores = score_sweeps({'age': age_scorer, 'gender': gender_scorer}, origin, sweeps, batch=16)
    r = dependency_ratio(scores['age']['p'], scores['gender']['p'])            # the age edit in p+: how much the gender moved with it
    feats = feature_sweeps(arcface.ArcFaceID('model_ir_se50.pth'), origin, sweeps, batch=16)
    d = identity_ratio(feats['p'], scores['age']['p'])                         # ... and how far the identity drifted per unit of age
"""
import numpy as np
import torch


def _scored(scorer, images, batch):
    out = [scorer(images[at:at + batch]).reshape(-1).float() for at in range(0, images.shape[0], batch)]
    return torch.cat(out)


@torch.no_grad()
def score_sweeps(scorers, origin, sweeps, batch):
    """scorers: {attribute: callable images [B,3,S,S] -> [B]}; origin [n,3,S,S]: the unedited images; sweeps: {space: [n,steps,3,S,S]}
    as edit_sweep returns them.  -> {attribute: {space: float32 numpy [n, steps + 1]}}: the first steps // 2 scores of the sweep, the
    origin's score, then the rest (editing_evaluate.py:176-190: three edits, the origin, three edits).  The images go through a
    scorer `batch` at a time."""
    if batch < 1:
        raise ValueError('score_sweeps: batch must be positive')
    if origin.ndim != 4:
        raise ValueError(f'score_sweeps: origin must be [n,3,S,S], got {tuple(origin.shape)}')
    n = origin.shape[0]
    for space, images in sweeps.items():
        if images.ndim != 5 or images.shape[0] != n or tuple(images.shape[2:]) != tuple(origin.shape[1:]):
            raise ValueError(f"score_sweeps: sweep '{space}' is {tuple(images.shape)}, expected [{n},steps,{','.join(map(str, origin.shape[1:]))}]")
    out = {}
    for attribute, scorer in scorers.items():
        mid = _scored(scorer, origin, batch).view(n, 1)
        out[attribute] = {}
        for space, images in sweeps.items():
            steps = images.shape[1]
            s = _scored(scorer, images.flatten(0, 1), batch).view(n, steps)
            out[attribute][space] = torch.cat([s[:, :steps // 2], mid.to(s.device), s[:, steps // 2:]], 1).cpu().numpy()
    return out


def dependency_ratio(change, interest):
    """calculate_score.py:52-71 for one (edited attribute, attribute of interest, space): change and interest are [M, 2h + 1] scores
    with the origin in column h (the reference's h is 3).  Per array, the positive side is sum(a[:, h+1:] - a[:, h:-1]) / M and the
    negative side sum(a[:, :h] - a[:, 1:h+1]) / M; -> (|interest+ / change+| + |interest- / change-|) / 2."""
    c, t = np.asarray(change, dtype=np.float64), np.asarray(interest, dtype=np.float64)
    if c.ndim != 2 or c.shape != t.shape or c.shape[1] < 3 or c.shape[1] % 2 == 0:
        raise ValueError(f'dependency_ratio: expected two [M, 2h + 1] arrays of one shape, got {c.shape} and {t.shape}')
    h, m = c.shape[1] // 2, c.shape[0]

    def sides(a):
        return np.sum(a[:, h + 1:] - a[:, h:-1]) / m, np.sum(a[:, :h] - a[:, 1:h + 1]) / m
    (cp, cn), (ip, in_) = sides(c), sides(t)
    return float((abs(ip / cp) + abs(in_ / cn)) / 2)


# ------------------------------------------------------------------------------------------------------ identity along a sweep
def _embedded(embed, images, batch):
    out = [embed(images[at:at + batch]) for at in range(0, images.shape[0], batch)]
    return torch.cat([f.reshape(f.shape[0], -1).float() for f in out])


@torch.no_grad()
def feature_sweeps(embed, origin, sweeps, batch):
    """embed: callable images [B,3,S,S] -> [B,D] (or anything that flattens to it: arcface.ArcFaceID, or
    inception_features.InceptionV3Features, the reference's own choice); origin [n,3,S,S]; sweeps: {space: [n,steps,3,S,S]} as edit_sweep
    returns them.  -> {space: float32 numpy [n, steps + 1, D]}: the first steps // 2 feature vectors of the sweep, the origin's, then
    the rest (our_interfaceGAN/editing_evaluate_id.py:174-193: three edits, the origin, three edits).  The images go through `embed`
    `batch` at a time."""
    if batch < 1:
        raise ValueError('feature_sweeps: batch must be positive')
    if origin.ndim != 4:
        raise ValueError(f'feature_sweeps: origin must be [n,3,S,S], got {tuple(origin.shape)}')
    n = origin.shape[0]
    for space, images in sweeps.items():
        if images.ndim != 5 or images.shape[0] != n or tuple(images.shape[2:]) != tuple(origin.shape[1:]):
            raise ValueError(f"feature_sweeps: sweep '{space}' is {tuple(images.shape)}, expected [{n},steps,{','.join(map(str, origin.shape[1:]))}]")
    mid = _embedded(embed, origin, batch).view(n, 1, -1)
    out = {}
    for space, images in sweeps.items():
        steps = images.shape[1]
        f = _embedded(embed, images.flatten(0, 1), batch).view(n, steps, -1)
        out[space] = torch.cat([f[:, :steps // 2], mid.to(f.device), f[:, steps // 2:]], 1).cpu().numpy()
    return out


def _cosine(a, b):
    """the cosine of the last axis, in fp64"""
    return np.sum(a * b, -1) / (np.sqrt(np.sum(a * a, -1)) * np.sqrt(np.sum(b * b, -1)))


def identity_similarity(features):
    """features [n, 2h + 1, D] as feature_sweeps lays them out -> float64 [n, 2h + 1]: every step's cosine to the origin column h, which
    is exactly 1 in that column"""
    f = np.asarray(features, dtype=np.float64)
    if f.ndim != 3 or f.shape[1] < 3 or f.shape[1] % 2 == 0:
        raise ValueError(f'identity_similarity: expected [n, 2h + 1, D] features, got {f.shape}')
    h = f.shape[1] // 2
    out = _cosine(f, f[:, h:h + 1])
    out[:, h] = 1.0                                          # a vector against itself: 1 by definition, not to rounding
    return out


def identity_ratio(features, change):
    """our_interfaceGAN/calculate_score_id.py:58-90 for one (edited attribute, space): features [M, 2h + 1, D] and the edited attribute's
    scores change [M, 2h + 1], the origin in column h (the reference's h is 3).  Unlike dependency_ratio each side has the end-to-origin
    term AND the h consecutive terms (:64-65 and :72-73 for the scores; :66-70 and :75-79 for the identity, whose terms are cosine
    DISTANCES, 1 - cos):
        change+ = sum_i ((c[i,2h] - c[i,h]) + sum(c[i,h+1:] - c[i,h:-1])) / M         change- likewise with c[i,0] and c[i,:h] - c[i,1:h+1]
        id+     = sum_i (d(f[i,2h], f[i,h]) + sum_j d(f[i,h+1+j], f[i,h+j])) / M      id- with d(f[i,0], f[i,h]) and d(f[i,j], f[i,j+1])
    -> (|id+ / change+| + |id- / change-|) / 2, in fp64."""
    f, c = np.asarray(features, dtype=np.float64), np.asarray(change, dtype=np.float64)
    if f.ndim != 3 or c.ndim != 2 or f.shape[:2] != c.shape or c.shape[1] < 3 or c.shape[1] % 2 == 0:
        raise ValueError(f'identity_ratio: expected [M, 2h + 1, D] features and [M, 2h + 1] scores, got {f.shape} and {c.shape}')
    h, m = c.shape[1] // 2, c.shape[0]

    def dist(a, b):
        return 1.0 - _cosine(a, b)
    cp = (np.sum(c[:, 2 * h] - c[:, h]) + np.sum(c[:, h + 1:] - c[:, h:-1])) / m
    cn = (np.sum(c[:, 0] - c[:, h]) + np.sum(c[:, :h] - c[:, 1:h + 1])) / m
    ip = (np.sum(dist(f[:, 2 * h], f[:, h])) + np.sum(dist(f[:, h + 1:], f[:, h:-1]))) / m
    in_ = (np.sum(dist(f[:, 0], f[:, h])) + np.sum(dist(f[:, :h], f[:, 1:h + 1]))) / m
    return float((abs(ip / cp) + abs(in_ / cn)) / 2)
