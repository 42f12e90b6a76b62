"""Evaluation of an attribute edit: the scores of the sweeps of transeditor_amd.edit.edit_sweep laid out as the reference's
our_interfaceGAN/editing_evaluate.py:164-196 lays them out, and the dependency figure of our_interfaceGAN/calculate_score.py:45-71 (how
much an attribute of interest moves while the edited attribute changes).  Host code on small arrays; the scorers run on the device.

    sweeps = edit.edit_sweep(G, z_plus, p_plus, zb, pb, z_distance=30, p_distance=30, steps=6, batch=16)
    scores = score_sweeps({'age': age_scorer, 'gender': gender_scorer}, origin, sweeps, batch=16)
    r = dependency_ratio(scores['age']['p'], scores['gender']['p'])            # the age edit in p+: how much the gender moved with it
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
