"""Host side of speaker diarization (the `spk_model` branch of FunASR's AutoModel), restated with numpy only.

  * `sv_chunk_bounds` / `sv_chunk`: 1.5-s windows with a 0.75-s hop over each VAD segment; the last window ends at the segment
    end, a segment shorter than a window gives one zero-padded window (funasr/models/campplus/utils.py `sv_chunk`).
  * `ClusterBackend`: fewer than 20 embeddings -> one speaker; fewer than 2048 -> spectral clustering (cosine affinity,
    p-pruning, symmetrised, unnormalised Laplacian, eigengap over 1..15 speakers or `oracle_num`, k-means on the eigenvectors);
    2048 or more with `oracle_num` -> k-means on L2-normalised embeddings; 2048 or more without it -> UMAP + HDBSCAN when
    `umap` and scikit-learn are importable; without `oracle_num` similar speakers are merged by centroid cosine afterwards
    (funasr/models/campplus/cluster_backend.py).
  * `postprocess` / `distribute_spk`: labels renumbered by first appearance, same-speaker neighbours merged, overlaps split in the
    middle, turns shorter than 0.7 s given to the nearer neighbour, then each sentence takes the speaker it overlaps most
    (campplus/utils.py `postprocess`, `distribute_spk`).
k-means is Lloyd's algorithm with k-means++ seeding from a fixed seed, so a call is reproducible.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

CHUNK_S = 1.5
SHIFT_S = 0.75


# ------------------------------------------------------------------------------------------------------------------ chunks
def sv_chunk_bounds(n: int, fs: int = 16000) -> List[Tuple[int, int]]:
    """(start, end) sample offsets of the windows over a segment of n samples"""
    size, hop = int(CHUNK_S * fs), int(SHIFT_S * fs)
    out: List[Tuple[int, int]] = []
    prev_end = 0
    for st in range(0, n, hop):
        end = min(st + size, n)
        if end <= prev_end:
            break
        prev_end = end
        out.append((max(0, end - size), end))
    return out


def sv_chunk(vad_segments: Sequence, fs: int = 16000) -> list:
    """[[start_s, end_s, samples], ...] segments -> [[chunk_start_s, chunk_end_s, window of int(1.5 fs) samples], ...]"""
    size = int(CHUNK_S * fs)
    res = []
    for seg_start, _, data in vad_segments:
        data = np.asarray(data)
        for st, end in sv_chunk_bounds(data.shape[0], fs):
            win = data[st:end]
            if win.shape[0] < size:
                win = np.concatenate([win, np.zeros(size - win.shape[0], dtype=win.dtype)])
            res.append([st / fs + seg_start, end / fs + seg_start, win])
    return res


# -------------------------------------------------------------------------------------------------------------- clustering
def _unit_rows(X: np.ndarray) -> np.ndarray:
    n = np.linalg.norm(X, axis=1, keepdims=True)
    return X / np.where(n == 0, 1.0, n)


def kmeans(X: np.ndarray, k: int, seed: int = 0, n_init: int = 10, max_iter: int = 300) -> np.ndarray:
    """Lloyd's k-means with k-means++ seeding; the best of n_init runs by inertia"""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    k = int(min(k, n))
    rng = np.random.default_rng(seed)
    best, best_in = None, np.inf
    for _ in range(n_init):
        centers = [X[rng.integers(n)]]
        for _ in range(1, k):
            d2 = np.min(((X[:, None, :] - np.asarray(centers)[None]) ** 2).sum(-1), axis=1)
            tot = d2.sum()
            centers.append(X[rng.choice(n, p=d2 / tot)] if tot > 0 else X[rng.integers(n)])
        C = np.asarray(centers)
        lab = np.zeros(n, dtype=np.int64)
        for it in range(max_iter):
            d = ((X[:, None, :] - C[None]) ** 2).sum(-1)
            new = d.argmin(1)
            if it > 0 and np.array_equal(new, lab):
                break
            lab = new
            for j in range(k):
                if np.any(lab == j):
                    C[j] = X[lab == j].mean(0)
        inertia = ((X - C[lab]) ** 2).sum()
        if inertia < best_in:
            best, best_in = lab.copy(), inertia
    return best


def spectral_labels(X: np.ndarray, oracle_num: Optional[int] = None, min_spks: int = 1, max_spks: int = 15,
                    pval: float = 0.022) -> np.ndarray:
    X = np.asarray(X, dtype=np.float64)
    U = _unit_rows(X)
    A = U @ U.T
    n = A.shape[0]
    p = 6.0 / n if n * pval < 6 else pval
    drop = int((1 - p) * n)                     # per row, the `drop` smallest affinities are set to 0
    order = np.argsort(A, axis=1, kind="stable")[:, :drop]
    np.put_along_axis(A, order, 0.0, axis=1)
    A = 0.5 * (A + A.T)
    np.fill_diagonal(A, 0.0)
    L = np.diag(np.abs(A).sum(1)) - A
    lam, vec = np.linalg.eigh(L)
    if oracle_num is not None:
        k = int(oracle_num)
    else:
        gaps = np.diff(lam[min_spks - 1: max_spks + 1])
        k = int(np.argmax(gaps)) + min_spks
    return kmeans(vec[:, :k], k)


def merge_by_cos(labels: np.ndarray, embs: np.ndarray, cos_thr: float) -> np.ndarray:
    """repeatedly fuse the two speakers whose centroids are most similar while that cosine is >= cos_thr"""
    if not 0 < cos_thr <= 1:
        raise ValueError("merge_by_cos: the threshold must lie in (0, 1]")
    labels = np.array(labels, copy=True)
    embs = np.asarray(embs, dtype=np.float64)
    while True:
        n_spk = int(labels.max()) + 1
        if n_spk == 1:
            break
        centers = _unit_rows(np.stack([embs[labels == i].mean(0) for i in range(n_spk)]))
        sim = np.triu(centers @ centers.T, 1)
        a, b = np.unravel_index(np.argmax(sim), sim.shape)
        if sim[a, b] < cos_thr:
            break
        labels = np.where(labels == b, a, labels)
        labels = np.where(labels > b, labels - 1, labels)
    return labels


class ClusterBackend:
    def __init__(self, merge_thr: float = 0.78, **kwargs):
        self.merge_thr = merge_thr

    def __call__(self, X, oracle_num: Optional[int] = None) -> np.ndarray:
        X = np.asarray(X, dtype=np.float64)
        if X.ndim != 2:
            raise ValueError("ClusterBackend: expected embeddings [N, C]")
        n = X.shape[0]
        if n < 20:
            return np.zeros(n, dtype=np.int64)
        if n < 2048:
            labels = spectral_labels(X, oracle_num)
        elif oracle_num is not None:
            labels = kmeans(_unit_rows(X), int(oracle_num))
        else:
            labels = self._umap_hdbscan(X)
        if oracle_num is None and self.merge_thr is not None:
            labels = merge_by_cos(labels, X, self.merge_thr)
        return labels

    @staticmethod
    def _umap_hdbscan(X: np.ndarray) -> np.ndarray:
        try:
            import umap.umap_ as umap
            from sklearn.cluster import HDBSCAN
        except ImportError as e:
            raise NotImplementedError(f"clustering 2048 or more speaker embeddings without preset_spk_num needs UMAP + HDBSCAN "
                                      f"({e.name or 'umap-learn / scikit-learn'} is not installed); pass preset_spk_num=<speakers> "
                                      "to cluster with k-means instead") from e
        Y = umap.UMAP(n_neighbors=20, min_dist=0.0, n_components=min(60, X.shape[0] - 2), metric="cosine").fit_transform(X)
        return HDBSCAN(min_samples=10, min_cluster_size=10, allow_single_cluster=True).fit_predict(Y)


# ------------------------------------------------------------------------------------------------------------ postprocess
def relabel_by_first_appearance(labels) -> np.ndarray:
    ids = {}
    return np.array([ids.setdefault(int(l), len(ids)) for l in labels], dtype=np.int64)


def _merge_runs(turns: list) -> list:
    out = [turns[0]]
    for t in turns[1:]:
        if t[2] == out[-1][2] and t[0] <= out[-1][1]:
            out[-1][1] = t[1]
        else:
            out.append(t)
    return out


def _smooth(turns: list, min_dur: float = 0.7) -> list:
    if len(turns) < 2:
        return turns
    last = len(turns) - 1
    for i, t in enumerate(turns):
        t[0], t[1] = round(t[0], 2), round(t[1], 2)
        if t[1] - t[0] >= min_dur:
            continue
        if i == 0:
            t[2] = turns[1][2]
        elif i == last:
            t[2] = turns[i - 1][2]
        else:
            t[2] = turns[i - 1][2] if t[0] - turns[i - 1][1] <= turns[i + 1][0] - t[1] else turns[i + 1][2]
    return _merge_runs(turns)


def postprocess(segments: list, vad_segments, labels, embeddings, return_spk_center: bool = False):
    """chunks [[start_s, end_s, ...], ...] + their labels -> speaker turns [[start_s, end_s, spk], ...] (and the per-speaker
    centroids of the embeddings, indexed by the renumbered speaker, with return_spk_center)"""
    if len(segments) != len(labels):
        raise ValueError("postprocess: one label per chunk")
    labels = relabel_by_first_appearance(labels)
    turns = _merge_runs([[s[0], s[1], l] for s, l in zip(segments, labels)])
    for i in range(1, len(turns)):
        if turns[i - 1][1] > turns[i][0] + 1e-4:                 # overlapping turns meet in the middle
            mid = (turns[i][0] + turns[i - 1][1]) / 2
            turns[i][0] = turns[i - 1][1] = mid
    turns = _smooth(turns)
    if return_spk_center:
        E = np.asarray(embeddings)
        return turns, np.stack([E[labels == i].mean(0) for i in range(int(labels.max()) + 1)])
    return turns


def distribute_spk(sentence_list: list, sd_time_list: list) -> list:
    """sentence["spk"] = the speaker whose turns overlap the sentence most; a speaker already leading gets each further
    overlapping turn counted twice, as the reference does"""
    turns = [(st * 1000, end * 1000, spk) for st, end, spk in sd_time_list]
    for sent in sentence_list:
        spk, score = 0, 0
        for st, end, who in turns:
            ov = max(min(sent["end"], end) - max(sent["start"], st), 0)
            if ov > score:
                score, spk = ov, who
            if ov > 0 and spk == who:
                score += ov
        sent["spk"] = int(spk)
    return sentence_list
