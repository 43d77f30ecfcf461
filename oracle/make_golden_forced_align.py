"""Golden vectors for the CTC forced alignment of SenseVoiceSmall's `output_timestamp` branch, made by the REFERENCE's own
`ctc_forced_align` (funasr/models/sense_voice/utils/ctc_alignment.py; build container only; TEST INFRASTRUCTURE). Writes
tests/golden/ctc_forced_align.npz: the frame labels it returns for the seeded random emission / target pairs of `cases()`,
which tests/test_sensevoice_timestamps.py regenerates from the same seed.

    python oracle/make_golden_forced_align.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import ref_import  # noqa: E402

GOLD = os.path.join(os.path.dirname(HERE), "tests", "golden", "ctc_forced_align.npz")


def cases(n=300, seed=0):
    """(log-probabilities [1, T, C], targets [1, L]) pairs that admit a path (a repeated target needs a blank between)."""
    g = torch.Generator().manual_seed(seed)
    for _ in range(n):
        T = int(torch.randint(1, 40, (1,), generator=g))
        C = int(torch.randint(3, 12, (1,), generator=g))
        L = int(torch.randint(1, max(2, min(T, 8) + 1), (1,), generator=g))
        lp = torch.log_softmax(torch.randn(1, T, C, generator=g) * 2, -1)
        tg = torch.randint(1, C, (1, L), generator=g)
        if L + int((tg[0, 1:] == tg[0, :-1]).sum()) > T:        # no valid path: the reference's output is unspecified
            continue
        yield lp, tg


def main():
    ref_import.install()
    from funasr.models.sense_voice.utils.ctc_alignment import ctc_forced_align as ref
    labels, lengths = [], []
    for lp, tg in cases():
        r = ref(lp.clone(), tg.clone(), torch.tensor([lp.shape[1]]), torch.tensor([tg.shape[1]]))[0].numpy()
        labels.append(r.astype(np.int32))
        lengths.append(len(r))
    np.savez_compressed(GOLD, labels=np.concatenate(labels), lengths=np.asarray(lengths, dtype=np.int32))
    print(f"{len(lengths)} cases -> {GOLD}")


if __name__ == "__main__":
    main()
