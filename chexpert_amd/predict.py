"""Prediction over a csv of image paths, as the reference's predict.py: probabilities of the five competition findings per study
(max over a study's views), from one checkpoint or the mean over the checkpoints of a folder, written as csv.  The forward pass is
the eval-mode HIP path of chexpert_amd.models; reading / cropping is chexpert_amd.data (mode 'test').

  python predict.py <data.csv> <predictions.csv> --restore_path <checkpoint.pt | folder> [--model densenet121|resnet152]
                    [--batch_size 16] [--resize N] [--mini_data N] [--cuda 0] [--tta K]
                    [--clahe [--clahe_grid GY GX] [--clahe_clip C]] [--calibration FILE]

--tta K averages the probabilities of K forwards per image: the image as decoded, and K - 1 random affine warps of it on the GPU
(chexpert_amd/augment.py, cx_u8_affine).  --clahe equalises every uint8 batch on the GPU first (ops.u8_clahe, as the training command
line's flag of the same name: a model trained with it is evaluated with it), before the forward and before each draw's warp.
--calibration FILE applies the per-class map stored in a calibration_<tag>.json of the training command line (chexpert_amd/calibration.py):
the probabilities are sigmoid(a z + b), under --tta before the mean over the K forwards.  Without the flag the output is unchanged.

A checkpoint of a `--uncertain multiclass` run (three logits per finding: negative, positive, uncertain) is recognised by its
classifier's row count: n rows build the usual head, 3n rows the wide one, whose logits are collapsed on the GPU right after every
forward (loss.collapse_multiclass: z = z_positive - z_negative, sigmoid(z) = p1 / (p0 + p1)); --calibration and --tta then act on z.
Any other count is an error, and the checkpoints of a folder must agree.  The pooling of the head (chexpert.py --pool) is read from
the checkpoint's `pool_state` (none: the average); the checkpoints of a folder must agree on it too.  The head (chexpert.py --head) is
read from the checkpoint's `head_state` (none: linear; csra or pcam) in the same way.

A checkpoint of a `--loss hier` run carries the parent table of its findings in `loss_state`: a table of 14 entries reads all 14
findings of the csv (one probability column each), and the conditional logits of every forward become unconditional ones on the GPU
(loss.collapse_hierarchy) before --calibration and --tta act on them.  The checkpoints of a folder must agree on the table.
"""
import argparse
import os

import numpy as np
import torch
import torch.nn as nn


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("data_path", type=str, help="csv with a Path column")
    p.add_argument("output_path", type=str, help="csv to write")
    p.add_argument("--restore_path", type=str, required=True, help="one checkpoint, or a folder of checkpoint*.pt to ensemble")
    p.add_argument("--model", default="densenet121", choices=["densenet121", "resnet152"])
    p.add_argument("--cuda", type=int, default=0)
    p.add_argument("--batch_size", type=int, default=16)
    p.add_argument("--resize", type=int)
    p.add_argument("--mini_data", type=int)
    p.add_argument("--tta", type=int, default=1, help="test-time augmentation: mean probability over K forwards (the image + K-1 affine warps)")
    p.add_argument("--tta_seed", type=int, default=0)
    p.add_argument("--clahe", action="store_true", help="CLAHE contrast equalisation of the uint8 image (GPU), as chexpert.py --clahe")
    p.add_argument("--clahe_grid", type=int, nargs=2, default=[8, 8], metavar=("GY", "GX"), help="tiles per axis, each 1..16, dividing the crop size")
    p.add_argument("--clahe_clip", type=float, default=2.0, metavar="C", help="clip limit in multiples of the mean bin height (0: no clipping)")
    p.add_argument("--calibration", default=None, metavar="FILE",
                   help="a calibration_<tag>.json written by chexpert.py --calibrate: the probabilities become sigmoid(a z + b)")
    return p


def parse_args(argv=None):
    """The command line; a --clahe grid that does not divide the crop size is refused here (parser.error)."""
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.clahe:
        from .augment import check_clahe_grid, clahe_clip_count
        size = args.resize or 320
        try:
            check_clahe_grid(args.clahe_grid, size, size)
            clahe_clip_count(args.clahe_clip, 1, 1)
        except ValueError as e:
            parser.error("--clahe: %s" % e)
    if args.calibration is not None and not os.path.isfile(args.calibration):
        parser.error("--calibration: no file %s" % args.calibration)
    return args


def probabilities(logits, cal=None):
    """The probabilities of a batch of logits: sigmoid(z) in fp32, or, with a fit (calibration.fit_calibration's dict, or what
    calibration.load_calibration reads), sigmoid(a z + b) with the per-class a, b rounded to fp32.  The identity map (a = 1, b = 0)
    gives the bits of the plain path: 1 * z + 0 is z."""
    z = logits.float()
    if cal is None:
        return torch.sigmoid(z)
    from .calibration import _map_of
    a, b = (torch.from_numpy(v.astype(np.float32)).to(z.device) for v in _map_of(cal, z.shape[-1]))
    return torch.sigmoid(z * a + b)


def head_is_multiclass(state_dict, key, n, path=""):
    """Whether the classifier `key` of a checkpoint's state_dict is the three-way head of a --uncertain multiclass run: False for n
    rows, True for 3n; any other count is a ValueError that names both."""
    rows = int(state_dict[key].shape[0])
    if rows not in (n, 3 * n):
        raise ValueError("checkpoint %s: %s has %d rows; the %d findings need %d (one logit each) or %d (three each: a --uncertain "
                         "multiclass run)" % (path, key, rows, n, n, 3 * n))
    return rows == 3 * n


def hier_parent_of(ck):
    """The parent table of a --loss hier checkpoint (its `loss_state`) as a list of ints; None for a checkpoint of another loss."""
    st = ck.get("loss_state") or {}
    if st.get("kind") != "hier":
        return None
    return [int(v) for v in torch.as_tensor(st["parent"]).tolist()]


@torch.no_grad()
def predict(model, dataset, batch_size, device, tta=1, tta_seed=0, clahe=None, cal=None, collapse=False):
    """DataFrame indexed by study ('.../patient64541/study1') with one probability column per finding (predict.py:33-52).

    tta = K > 1 (test-time augmentation): per image the mean of K sigmoid probabilities, then the max over a study's views as
    before.  Draw 0 is the batch as decoded; draws 1 .. K-1 warp the uint8 batch with ops.u8_affine (fill 0) and matrices from
    augment.affine_matrices at half the ranges of the training defaults -- rotation +-5 degrees, translation +-0.025 of the size,
    scale 0.95 .. 1.05, no shear (augment.TTA_RANGES) -- seeded by augment.tta_seed_of(tta_seed, draw, number of the minibatch):
    two calls agree bit for bit.  tta = 1 is the plain path.

    clahe: an augment.Clahe (or None): the uint8 batch is equalised once on the GPU, before the forward and before each draw's warp.
    cal: a calibration fit (or None): every forward's probabilities are sigmoid(a z + b) (`probabilities`), before the mean over the draws.
    collapse: the model has the three-way head of a --uncertain multiclass run; every forward's (B, 3n) logits become the binary
    z = z_positive - z_negative (loss.collapse_multiclass) before `probabilities`.  A parent table as `collapse`: the model was trained
    with the hierarchical loss; every forward's conditional logits become unconditional ones (loss.collapse_hierarchy) there."""
    import pandas as pd
    from .data import extract_patient_ids
    if tta < 1:
        raise ValueError("tta must be >= 1")
    model.eval()
    forward = model
    if collapse is True:
        from .loss import collapse_multiclass

        def forward(xb):
            return collapse_multiclass(model(xb))
    elif collapse:
        from .loss import collapse_hierarchy
        from .ops import check_hier_parent
        table = collapse if isinstance(collapse, torch.Tensor) and collapse.is_cuda else check_hier_parent("predict", collapse).to(device)

        def forward(xb):
            return collapse_hierarchy(model(xb), table)
    probs, studies = [], []
    for k in range(0, len(dataset), batch_size):
        items = [dataset[i] for i in range(k, min(k + batch_size, len(dataset)))]
        x = torch.stack([it[0] for it in items]).to(device)
        if clahe is not None:
            x = clahe(x)
        if tta == 1:
            probs.append(probabilities(forward(x), cal).cpu())
        else:
            from . import augment, ops
            if x.dtype != torch.uint8:
                raise RuntimeError("test-time augmentation warps the decoded uint8 images (got %s)" % x.dtype)
            p = probabilities(forward(x), cal)
            for draw in range(1, tta):
                mat = augment.affine_matrices(augment.tta_seed_of(tta_seed, draw, k // batch_size), x.shape[0], x.shape[-2], x.shape[-1],
                                              **augment.TTA_RANGES)
                p = p + probabilities(forward(ops.u8_affine(x, mat.to(device))), cal)
            probs.append((p / tta).cpu())
        studies += list(extract_patient_ids(dataset, [it[2] for it in items]))
    df = pd.DataFrame(torch.cat(probs).numpy(), index=studies, columns=list(dataset.attr_names))
    df.index.name = "Study"
    return df.groupby("Study").max()


def main(argv=None):
    import pandas as pd
    from .data import ChexpertCSV
    from .models import densenet121, resnet152
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("predict runs on the GPU only (there is no CPU path)")
    device = torch.device("cuda:%d" % args.cuda)
    key = "classifier.weight" if args.model == "densenet121" else "fc.weight"

    def build(width, pool_state, head_state):
        if args.model == "densenet121":
            net = densenet121(pretrained=False)
            net.classifier = nn.Linear(net.classifier.in_features, width)
        else:
            net = resnet152(pretrained=False)
            net.fc = nn.Linear(net.fc.in_features, width)
        return net.to(device).load_pool_state(pool_state).load_head_state(head_state)
    if os.path.isdir(args.restore_path):
        files = sorted(os.path.join(args.restore_path, f) for f in os.listdir(args.restore_path)
                       if f.startswith("checkpoint") and f.endswith(".pt"))
        print("Running ensemble prediction using %d checkpoints." % len(files))
    else:
        files = [args.restore_path]
    # a --loss hier checkpoint carries its parent table (`loss_state`): the table says how many findings the run read (14: --labels
    # all) and how the conditional logits are collapsed; the checkpoints of a folder must agree on it
    from .data import ATTR_NAMES, ATTR_NAMES_ALL
    first = torch.load(files[0], map_location=device)
    parent = hier_parent_of(first)
    if parent is not None and len(parent) not in (len(ATTR_NAMES), len(ATTR_NAMES_ALL)):
        raise ValueError("checkpoint %s: its parent table has %d entries; predict reads the %d competition findings or all %d"
                         % (files[0], len(parent), len(ATTR_NAMES), len(ATTR_NAMES_ALL)))
    ds = ChexpertCSV(args.data_path, "test", args.resize, mini_data=args.mini_data,
                     labels="all" if parent is not None and len(parent) == len(ATTR_NAMES_ALL) else "competition")
    n = len(ds.attr_names)
    frames = []
    clahe = None
    if args.clahe:
        from .augment import Clahe
        clahe = Clahe(args.clahe_grid, args.clahe_clip)
    cal = None
    if args.calibration is not None:
        from .calibration import load_calibration
        cal = load_calibration(args.calibration)
    model = wide = None
    for f in files:
        ck = first if f == files[0] else torch.load(f, map_location=device)
        sd, pool_kind = ck["state_dict"], (ck.get("pool_state") or {}).get("kind", "avg")
        head_kind = (ck.get("head_state") or {}).get("kind", "linear")
        w = head_is_multiclass(sd, key, n, f)
        if hier_parent_of(ck) != parent:
            raise ValueError("the checkpoints of %s disagree: %s has the parent table %s, %s has %s (None: no hierarchical loss)"
                             % (args.restore_path, files[0], parent, f, hier_parent_of(ck)))
        if model is None:                   # the first checkpoint's head decides; the others of a folder must agree
            model, wide = build(n * (3 if w else 1), ck.get("pool_state"), ck.get("head_state")), w
        elif head_kind != model.head_kind:
            raise ValueError("the checkpoints of %s disagree: %s has the %s head, %s the %s head" % (args.restore_path, files[0], model.head_kind,
                                                                                                f, head_kind))
        elif pool_kind != model.pool_kind:
            raise ValueError("the checkpoints of %s disagree: %s pools with %s, %s with %s" % (args.restore_path, files[0], model.pool_kind,
                                                                                          f, pool_kind))
        elif w != wide:
            raise ValueError("the checkpoints of %s disagree: %s has %d logits per finding, %s has %d" % (args.restore_path, files[0],
                                                                                                       3 if wide else 1, f, 3 if w else 1))
        model.load_state_dict(sd)
        frames.append(predict(model, ds, args.batch_size, device, tta=args.tta, tta_seed=args.tta_seed, clahe=clahe, cal=cal,
                              collapse=wide if parent is None else parent))
    df = frames[0] if len(frames) == 1 else sum(frames[1:], frames[0]) / float(len(frames))      # mean over checkpoints
    df.to_csv(args.output_path)
    return df


if __name__ == "__main__":
    main()
