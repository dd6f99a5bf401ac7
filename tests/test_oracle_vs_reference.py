"""Oracle pinned against the reference's own train steps: tests/golden/ref_step_<net>.npz, written by the imported reference
(oracle/make_ref_steps_golden.py, which also checks the SURVEY.md section 8c anchor of the reference against the oracle)."""
import os
import warnings

import numpy as np
import pytest
import torch

import cdnet_ref as O


@pytest.fixture(scope="module")
def ref(golden_dir):
    """the fixtures, with the oracle run at the thread count they were written at (oracle/make_ref_steps_golden.py THREADS: the
    summation order of the CPU convolutions follows it, and AdamW magnifies that on near-zero gradients)"""
    threads = torch.get_num_threads()
    torch.set_num_threads(8)

    def load(name):
        with np.load(os.path.join(golden_dir, "ref_step_%s.npz" % name)) as z:
            return {k: z[k] for k in z.files}
    yield load
    torch.set_num_threads(threads)


def _close(row, got, tol, rel, what=""):
    """got against a stored row (oracle/make_ref_steps_golden.py): its elements at the stored flat indices within tol
    (+ rel x the reference's max |x|), its max |x| within the same bound, its norm within 1e-5 relative"""
    v = got.detach().reshape(-1).double().numpy()
    m = row.size - 2
    k = min(m, v.size)
    want, mx, nrm = row[:k].astype(np.float64), float(row[m]), float(row[m + 1])
    assert np.isfinite(want).all() and np.isnan(row[k:m]).all(), what
    bound = tol + rel * mx
    assert float(np.abs(v[np.linspace(0, v.size - 1, k).astype(np.int64)] - want).max()) <= bound, what
    assert abs(float(np.abs(v).max()) - mx) <= bound, what
    assert abs(float(np.linalg.norm(v)) - nrm) <= 1e-5 * nrm + 1e-9, what


@pytest.mark.parametrize("name", ["base_transformer_pos_s4", "base_transformer_pos_s4_dd8_t8_e2d4",
                                  "base_transformer_pos_s4_resnet50"])
def test_train_step_equals_reference(name, ref):
    """logits, focal loss, every gradient and two AdamW updates vs models/networks.py +
    models/losses.py + torch.optim.AdamW (models/trainer.py:39-40,302-308)."""
    cfg = O.get_config(name)
    st = O.TrainState(name, O.deterministic_state(name), lr=0.01)
    a, b, lab = O.synthetic_batch(3, 64, seed=7, n_class=cfg["n_class"])
    r = ref(name)
    for it in range(2):
        yo, lo = st.step(a, b, lab)
        _close(r["logits%d" % it], yo, 0.0, 1e-5, "logits")
        assert abs(float(r["loss%d" % it]) - lo) < 1e-6
        for k, g, p in zip(r["keys"], r["grad%d" % it], r["param%d" % it]):      # the reference's named_parameters()
            q = st.sd[k]
            assert np.isnan(g[-1]) == (q.grad is None), k
            if q.grad is not None:
                _close(g, q.grad, 1e-9, 1e-5, k)
            _close(p, q, 1e-5, 0.0, k)


def test_xbd_train_step_equals_reference(ref):
    """xBD copy (xBD_code/zoo/model_transformer_encoding.py), ComboLoss (xBD_code/losses.py), clip_grad_norm_ and the
    hand-rolled AdamW (xBD_code/adamw.py) exactly as xBD_code/train.py:331-374 chains them; with_decoder_pos=None so that
    a 256x256 input runs (the 'learned' variant is pinned at 1024x1024 through the golden fixture)."""
    name = "xbd_unet_transformer_nodecpos"
    sd = O.deterministic_state(name)
    a, b, lab = O.synthetic_batch(2, 256, seed=21, n_class=5)
    x6, msk = torch.cat([a, b], 1), O.xbd_masks(lab)
    st = O.XbdTrainState(name, sd)
    r = ref(name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for it in range(2):
            yo, lo = st.step(x6, msk)
            _close(r["logits%d" % it], yo, 0.0, 1e-5, "logits")
            want = float(r["loss%d" % it])
            assert abs(want - lo) <= 1e-6 * want
            tn = float(r["total_norm%d" % it])
            assert abs(tn - st.last_total_norm) <= 1e-5 * tn
            for k, p in zip(r["keys"], r["param%d" % it]):
                _close(p, st.sd[k], 1e-6, 0.0, k)
