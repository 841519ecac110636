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


@torch.no_grad()
def predict(model, dataset, batch_size, device, tta=1, tta_seed=0, clahe=None, cal=None):
    """DataFrame indexed by study ('.../patient64541/study1') with one probability column per finding (predict.py:33-52).

    tta = K > 1 (test-time augmentation): per image the mean of K sigmoid probabilities, then the max over a study's views as
    before.  Draw 0 is the batch as decoded; draws 1 .. K-1 warp the uint8 batch with ops.u8_affine (fill 0) and matrices from
    augment.affine_matrices at half the ranges of the training defaults -- rotation +-5 degrees, translation +-0.025 of the size,
    scale 0.95 .. 1.05, no shear (augment.TTA_RANGES) -- seeded by augment.tta_seed_of(tta_seed, draw, number of the minibatch):
    two calls agree bit for bit.  tta = 1 is the plain path.

    clahe: an augment.Clahe (or None): the uint8 batch is equalised once on the GPU, before the forward and before each draw's warp.
    cal: a calibration fit (or None): every forward's probabilities are sigmoid(a z + b) (`probabilities`), before the mean over the draws."""
    import pandas as pd
    from .data import extract_patient_ids
    if tta < 1:
        raise ValueError("tta must be >= 1")
    model.eval()
    probs, studies = [], []
    for k in range(0, len(dataset), batch_size):
        items = [dataset[i] for i in range(k, min(k + batch_size, len(dataset)))]
        x = torch.stack([it[0] for it in items]).to(device)
        if clahe is not None:
            x = clahe(x)
        if tta == 1:
            probs.append(probabilities(model(x), cal).cpu())
        else:
            from . import augment, ops
            if x.dtype != torch.uint8:
                raise RuntimeError("test-time augmentation warps the decoded uint8 images (got %s)" % x.dtype)
            p = probabilities(model(x), cal)
            for draw in range(1, tta):
                mat = augment.affine_matrices(augment.tta_seed_of(tta_seed, draw, k // batch_size), x.shape[0], x.shape[-2], x.shape[-1],
                                              **augment.TTA_RANGES)
                p = p + probabilities(model(ops.u8_affine(x, mat.to(device))), cal)
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
    ds = ChexpertCSV(args.data_path, "test", args.resize, mini_data=args.mini_data)
    n = len(ds.attr_names)
    if args.model == "densenet121":
        model = densenet121(pretrained=False)
        model.classifier = nn.Linear(model.classifier.in_features, n)
    else:
        model = resnet152(pretrained=False)
        model.fc = nn.Linear(model.fc.in_features, n)
    model = model.to(device)
    if os.path.isdir(args.restore_path):
        files = sorted(os.path.join(args.restore_path, f) for f in os.listdir(args.restore_path)
                       if f.startswith("checkpoint") and f.endswith(".pt"))
        print("Running ensemble prediction using %d checkpoints." % len(files))
    else:
        files = [args.restore_path]
    frames = []
    clahe = None
    if args.clahe:
        from .augment import Clahe
        clahe = Clahe(args.clahe_grid, args.clahe_clip)
    cal = None
    if args.calibration is not None:
        from .calibration import load_calibration
        cal = load_calibration(args.calibration)
    for f in files:
        model.load_state_dict(torch.load(f, map_location=device)["state_dict"])
        frames.append(predict(model, ds, args.batch_size, device, tta=args.tta, tta_seed=args.tta_seed, clahe=clahe, cal=cal))
    df = frames[0] if len(frames) == 1 else sum(frames[1:], frames[0]) / float(len(frames))      # mean over checkpoints
    df.to_csv(args.output_path)
    return df


if __name__ == "__main__":
    main()
