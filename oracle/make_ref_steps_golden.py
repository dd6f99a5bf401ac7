"""Generate tests/golden/ref_step_<net>.npz FROM THE REFERENCE ITSELF (container-only; needs the reference tree, see ref_import).

    python oracle/make_ref_steps_golden.py

Two train steps of the reference exactly as tests/test_oracle_vs_reference.py replays them with the oracle:
  base_transformer_pos_s4, base_transformer_pos_s4_dd8_t8_e2d4, base_transformer_pos_s4_resnet50 -- models/networks.py +
      models/losses.py focal_loss + torch.optim.AdamW (models/trainer.py:39-40,302-308), batch 3 at 64x64, seed 7, lr 0.01
  xbd_unet_transformer_nodecpos -- xBD_code ComboLoss + clip_grad_norm_ + its AdamW (xBD_code/train.py:331-374),
      batch 2 at 256x256, seed 21
Per step: the loss, the logits, every parameter gradient and every parameter after the update, all at THREADS CPU threads.
A tensor of n elements is stored as one row: its elements at the flat indices linspace(0, n - 1, min(n, m)) (m = SAMPLE, the
logits LOGIT_SAMPLE; NaN-padded to m), then its max |x| and its norm -- a tensor of up to m elements in full.  `keys` lists
the reference's named_parameters() in order; a parameter without a gradient has a row of NaN in grad<step>.  Before writing, the SURVEY.md section 8c anchor of the reference is checked (define_G
under torch.manual_seed(0), s4 eval: logits sum -415.798811, the oracle's forward on those weights within 1e-6).
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cdnet_ref as O          # noqa: E402  (only for the input / weight generators and the anchor)
import ref_import              # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden", "ref_step_%s.npz")
BIT_NETS = ("base_transformer_pos_s4", "base_transformer_pos_s4_dd8_t8_e2d4", "base_transformer_pos_s4_resnet50")
XBD_NET = "xbd_unet_transformer_nodecpos"
SAMPLE = 32
LOGIT_SAMPLE = 1024
THREADS = 8      # CPU convolutions sum in an order that follows the thread count; AdamW turns that into whole lr-sized steps on
                 # near-zero gradients, so the tests replay the oracle at the same count


def _row(t, m=SAMPLE):
    row = np.full(m + 2, np.nan)
    if t is None:
        return row
    v = t.detach().reshape(-1).double().numpy()
    k = min(m, v.size)
    row[:k] = v[np.linspace(0, v.size - 1, k).astype(np.int64)]
    row[m], row[m + 1] = np.abs(v).max(), np.linalg.norm(v)
    return row


def _save(name, net, rec):
    rec["keys"] = np.array([k for k, _ in net.named_parameters()])
    np.savez_compressed(OUT % name, **{k: (v.astype(np.float32) if v.dtype == np.float64 and v.ndim else v)
                                       for k, v in rec.items()})
    print(name, os.path.getsize(OUT % name), "bytes")


def _anchor():
    torch.manual_seed(0)
    net = ref_import.define_G("base_transformer_pos_s4").eval()
    g = torch.Generator().manual_seed(1)
    a = torch.randn(2, 3, 256, 256, generator=g)
    b = torch.randn(2, 3, 256, 256, generator=g)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        y = net(a, b)
        yo = O.forward(sd, "base_transformer_pos_s4", a, b, training=False)
    assert abs(float(y.sum()) - (-415.798811)) < 1e-2
    assert float((y - yo).abs().max()) <= 1e-6


def main():
    torch.set_num_threads(THREADS)
    _anchor()
    _, ref_losses = ref_import.load()
    for name in BIT_NETS:
        cfg = O.get_config(name)
        net = ref_import.build_resnet50_variant() if cfg.get("backbone") == "resnet50" else ref_import.define_G(name)
        net.load_state_dict(O.deterministic_state(name))
        net.train()
        opt = torch.optim.AdamW(net.parameters(), lr=0.01, betas=(0.9, 0.999), weight_decay=0.01)
        a, b, lab = O.synthetic_batch(3, 64, seed=7, n_class=cfg["n_class"])
        rec = {}
        for it in range(2):
            y = net(a, b)
            opt.zero_grad()
            loss = ref_losses.focal_loss(y, lab)
            loss.backward()
            opt.step()
            rec["logits%d" % it] = _row(y, LOGIT_SAMPLE)
            rec["loss%d" % it] = np.float64(loss.item())
            rec["grad%d" % it] = np.stack([_row(p.grad) for _, p in net.named_parameters()])
            rec["param%d" % it] = np.stack([_row(p) for _, p in net.named_parameters()])
        _save(name, net, rec)

    _, xlosses, xadamw = ref_import.load_xbd()
    net = ref_import.build_xbd_model(None)
    net.load_state_dict(O.deterministic_state(XBD_NET))
    net.train()
    a, b, lab = O.synthetic_batch(2, 256, seed=21, n_class=5)
    x6, msk = torch.cat([a, b], 1), O.xbd_masks(lab)
    opt = xadamw.AdamW(net.parameters(), lr=1e-4, weight_decay=1e-6)
    seg = xlosses.ComboLoss({'dice': 1, 'focal': 8}, per_image=False)
    rec = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for it in range(2):
            net.zero_grad()
            out = net(x6)
            loss = sum(w * seg(out[:, c], msk[:, c]) for c, w in enumerate(O.XBD_CHANNEL_WEIGHTS))
            loss.backward()
            tn = torch.nn.utils.clip_grad_norm_(net.parameters(), 0.999)
            opt.step()
            rec["logits%d" % it] = _row(out, LOGIT_SAMPLE)
            rec["loss%d" % it] = np.float64(loss.item())
            rec["total_norm%d" % it] = np.float64(tn.item())
            rec["param%d" % it] = np.stack([_row(p) for _, p in net.named_parameters()])
    _save(XBD_NET, net, rec)


if __name__ == "__main__":
    main()
