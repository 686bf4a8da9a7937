#!/usr/bin/env python3
"""Evaluation entry point -- the reference's test.py (calc_acc :31-252, main :255-298) on the HIP path.

    python test.py --curObj LPW --path2data ... --loadfile ... --setting configs/baseline_edge.yaml
    python test.py --synthetic 16 --batchsize 8 --setting configs/baseline_edge.yaml      # no data needed
"""
import os
import pickle
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import egne_amd  # noqa: E402,F401
from egne_amd import _entry, parallel  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

from egne_amd.args import ellipse_metrics_note, parse_args  # noqa: E402
from egne_amd.utils import calc_edge, getPoint_metric, getSeg_metrics  # noqa: E402


def calc_acc(args, testloader, model, edge_model, device):
    """test.py:31-252: per batch edge -> model -> argmax -> metrics; with --disp 1 the overlay grid of every batch (test.py:165-181) goes
    to a JPEG file instead of a window."""
    ious, dists_pupil_latent, dists_pupil_seg, dists_iris_latent, dists_iris_seg, losses = [], [], [], [], [], []
    model.eval()
    # the edge network of batch i+1 runs next to the model of batch i (egne_amd.pipeline), and the host computes the metrics of
    # batch i-1 meanwhile: same numbers, one batch later
    from egne_amd.pipeline import TwoStagePipeline
    pipe = TwoStagePipeline(args, edge_model, torch.device(device))
    waiting = []
    ledger = None
    if getattr(args, "device_metrics", 0):
        # --device_metrics 1: the class map and the labels stay on the device; one row of raw scores per sample (egne_amd.scores), one
        # copy down behind the last batch.  DeepVOG predicts pupil / not pupil: two classes against labels == 2 (test.py:157-158)
        from egne_amd import scores
        ledger = scores.ScoreLedger(len(testloader) * args.batchsize, device, ncls=2 if args.model == 'deepvog' else 3)
    elif getattr(args, "record_iou", 0):
        print('--record_iou 1 needs --device_metrics 1: the per-sample IoUs are rows of its ledger; nothing is written')
    # --ellipse_metrics 1: the block the reference keeps behind bbox_iou_flag (test.py:108-155), one more row per sample on the device.
    # DeepVOG predicts the pupil only, as class 1 of its two-class map: the iris columns stay NaN
    ell_ledger = None
    calc_acc.last_ellipse_summary = None
    note = ellipse_metrics_note(args)
    if note:
        print(note)
    elif getattr(args, "ellipse_metrics", 0):
        ell_ledger = scores.EllipseLedger(len(testloader) * args.batchsize, device, classes=(-1, 1) if args.model == 'deepvog' else (1, 2))

    def second(batch):
        img, labels, spatialWeights, distMap, pupil_center, iris_center, elNorm, cond, imInfo = batch

        def run(img_edge):
            with torch.no_grad():
                op, elPred, _, loss, elOut = model(img.to(device).to(args.prec), img_edge, labels.to(device).long(),
                                                   pupil_center.to(device).to(args.prec), elNorm.to(device).to(args.prec),
                                                   spatialWeights.to(device).to(args.prec), distMap.to(device).to(args.prec),
                                                   cond.to(device).to(args.prec), imInfo[:, 2].to(device).to(torch.long), 0.5)
                return model.predictions().clone(), elPred, elOut, loss, model.loss_flags()      # device argmax == get_predictions(op) (utils.py:65-81)
        return run

    redo = [False]
    disp_dir = None
    if getattr(args, "disp", 0) and parallel.rank() == 0:
        # --disp 1: the grid the reference shows for every batch (test.py:165-181: elPred, override, elNorm), drawn and encoded on the
        # device (egne_amd.dispgrid), one file per batch
        from egne_amd import dispgrid
        disp_dir = os.path.join('img', '{}_{}_disp'.format(args.curObj if args.curObj is not None else 'synthetic', args.method))
        os.makedirs(disp_dir, exist_ok=True)
    drawn = [0]

    def metrics(batch, r):
        (mask, elPred, elOut, loss, flags), done = r
        done.synchronize()
        # both words are read (and cleared) before they are combined: an edge-network overflow puts NaNs into the edge map, so the
        # model's plan flags too, and a short-circuit `or` would leave the edge plan's word set and its stale scales in place
        ov = bool(model.overflowed()) | bool(edge_model.overflowed())
        if redo[0] or ov:
            # a frame beyond the head-room of the calibrated f16 pre-scales (engine.Plan.overflowed): the results of this batch are
            # invalid; a plan re-calibrates on its next call, so the batch runs again, back to back.  The batch queued behind it ran its
            # edge network with the old scales, and its flag went with the words cleared here: whenever a batch cleared a word, the next
            # one runs again as well.  Up to three attempts: the word may have been set by the NEXT batch's edge network (already running), in
            # which case this batch re-calibrates the plans on ITS frames and the next one overflows them once more
            cleared = ov
            torch.cuda.synchronize()    # the edge network of the NEXT batch is in flight on the pipeline's stream and owns the same plan buffers
            for attempt in (0, 1, 2):
                with torch.no_grad():
                    edge = calc_edge(args, batch[0].to(device), edge_model, device)
                    again = bool(edge_model.overflowed())
                    if not again:           # (a NaN edge map must not reach the model plan's own calibration pass)
                        mask, elPred, elOut, loss, flags = second(batch)(edge)
                        torch.cuda.synchronize()
                        again = bool(model.overflowed())
                if not again:
                    break
                cleared = True
            else:
                raise RuntimeError("non-finite activations after re-calibration: the input frames themselves are not finite")
            redo[0] = cleared
        model.raise_on_loss_flags(flags)           # two absent classes: loss.py:132 raises in the reference
        img, labels, spatialWeights, distMap, pupil_center, iris_center, elNorm, cond, imInfo = batch
        if disp_dir is not None:    # behind the redo decision: a batch that ran again is drawn once, with its second result
            u8 = dispgrid.script_grid(args.model, img.to(device), mask, elPred, cond.to(device), elNorm.to(device), override=True)
            dispgrid.save_grid(os.path.join(disp_dir, 'batch_%05d.jpg' % drawn[0]), u8)
            drawn[0] += 1
        if ledger is not None:      # behind the redo decision: a batch that ran again is counted once, with its second result
            lab = labels.to(device).long()
            ledger.append((lab == 2).long() if ledger.ncls == 2 else lab, mask, elOut, elPred, pupil_center.to(device), iris_center.to(device),
                          elNorm.to(device), cond.to(device), loss)
            if ell_ledger is not None:
                ell_ledger.append(mask, elPred, elNorm.to(device), cond.to(device), search=bool(args.ellipse_search))
            return
        predict = mask.cpu().numpy()
        cnp = cond.cpu().numpy().astype(np.float32)
        iou, _, _ = getSeg_metrics(labels.cpu().numpy(), predict, cnp[:, 1])
        H, W = labels.shape[1:]
        pupil_c, iris_c = pupil_center.cpu().numpy(), iris_center.cpu().numpy()       # (device tensors under --device_loader 1)
        lat_p, _ = getPoint_metric(pupil_c, elOut[:, 5:7].cpu().numpy(), cnp[:, 0], (H, W), True)
        seg_p, _ = getPoint_metric(pupil_c, elPred[:, 5:7].cpu().numpy(), cnp[:, 0], (H, W), True)
        lat_i, _ = getPoint_metric(iris_c, elOut[:, 0:2].cpu().numpy(), cnp[:, 1], (H, W), True)
        seg_i, _ = getPoint_metric(iris_c, elPred[:, 0:2].cpu().numpy(), cnp[:, 1], (H, W), True)
        ious.append(iou)
        dists_pupil_latent.append(lat_p); dists_pupil_seg.append(seg_p)
        dists_iris_latent.append(lat_i); dists_iris_seg.append(seg_i)
        losses.append(loss.mean().item())

    for bt, batch in enumerate(testloader):
        if args.test_normal and bt > 20:       # test.py:76
            break
        if args.device_loader:                 # a RawBatch: the nine tensors are built on the GPU (egne_amd.loader), no augmentation
            from egne_amd import loader
            from egne_amd.args import loader_geometry
            size, scale = loader_geometry(args)
            batch = loader.device_batch(batch, size=size, scale=scale, augment=False)
        waiting.append(batch)
        r = pipe.submit(batch[0].to(device), second(batch))
        if r is not None:
            metrics(waiting.pop(0), r)
    r = pipe.flush()
    if r is not None and waiting:
        metrics(waiting.pop(0), r)
    assert not waiting
    if ledger is not None:
        # the same per-batch numbers from the rows: utils.getSeg_metrics' own reduction, the flag / sum / divide of getPoint_metric, the
        # float32 loss widened as .item() widens it
        rows = scores.gather_rows(ledger.rows())
        for b in scores.batches(rows):
            ious.append(scores.seg_metrics(b)[0])
            dists_pupil_latent.append(scores.point_metric(b, "pupil_latent", 0)[0]); dists_pupil_seg.append(scores.point_metric(b, "pupil_seg", 0)[0])
            dists_iris_latent.append(scores.point_metric(b, "iris_latent", 1)[0]); dists_iris_seg.append(scores.point_metric(b, "iris_seg", 1)[0])
            losses.append(float(b[0, scores.LOSS]))
        if args.record_iou and parallel.rank() == 0:          # test.py:219-230
            os.makedirs('img', exist_ok=True)
            filename = os.path.join('img', '{}_{}_ious.pkl'.format(args.curObj if args.curObj is not None else 'synthetic', args.method))
            with open(filename, 'wb') as f:
                pickle.dump(np.ascontiguousarray(rows[:, scores.IOU:scores.IOU + 3]), f)
            print('per-sample IoUs {} written to {}'.format(rows[:, scores.IOU:scores.IOU + 3].shape, filename))
        if ell_ledger is not None:
            ell_rows = scores.gather_rows(ell_ledger.rows(), scores.ELL_FIELDS, scores.ELL_BATCH)
            calc_acc.last_ellipse_summary = scores.ellipse_summary(ell_rows)
            if args.record_iou and parallel.rank() == 0:      # the job of the reference's record_new_parameters (test.py:142-147)
                filename = os.path.join('img', '{}_{}_ellipses.pkl'.format(args.curObj if args.curObj is not None else 'synthetic', args.method))
                with open(filename, 'wb') as f:
                    pickle.dump({'fields': scores.ell_field_names(), 'rows': np.ascontiguousarray(ell_rows)}, f)
                print('per-sample ellipse scores {} written to {}'.format(ell_rows.shape, filename))
    elif parallel.world_size() > 1:     # frames shard over ranks (no data-path collective); only the per-batch metrics are gathered
        ious, dists_pupil_latent, dists_pupil_seg, dists_iris_latent, dists_iris_seg, losses = (
            parallel.gather_lists(v) for v in (ious, dists_pupil_latent, dists_pupil_seg, dists_iris_latent, dists_iris_seg, losses))
    ious = np.nanmean(np.stack(ious)) if ious else np.nan
    if parallel.world_size() > 1 and torch.distributed.get_rank() != 0:
        return ious, np.nanmedian(dists_pupil_seg), np.nanmedian(dists_iris_seg), float(np.mean(losses))
    print('mIoU: {}'.format(ious))
    print('Latent space PUPIL dist. Med: {}, STD: {}'.format(np.nanmedian(dists_pupil_latent), np.nanstd(dists_pupil_latent)))
    print('Segmentation PUPIL dist. Med: {}, STD: {}'.format(np.nanmedian(dists_pupil_seg), np.nanstd(dists_pupil_seg)))
    print('Latent space IRIS dist. Med: {}, STD: {}'.format(np.nanmedian(dists_iris_latent), np.nanstd(dists_iris_latent)))
    print('Segmentation IRIS dist. Med: {}, STD: {}'.format(np.nanmedian(dists_iris_seg), np.nanstd(dists_iris_seg)))
    if calc_acc.last_ellipse_summary is not None:
        s = calc_acc.last_ellipse_summary
        has_iris = args.model != 'deepvog'
        print('Bounding box Pupil IoU. Mean : {}'.format(s['bbiou_pupil']))         # test.py:240-247
        if has_iris: print('Bounding box Iris IoU. Mean : {}'.format(s['bbiou_iris']))
        print('ABS Pupil parameters : ', s['para_pupil'])
        if has_iris: print('ABS Iris parameters : ', s['para_iris'])
        for name in (('pupil', 'iris') if has_iris else ('pupil',)):
            print('Ellipse area {} IoU against ground truth. Mean : {}'.format(name.upper(), s['ell_iou_' + name]))
            print('Class map {} IoU. Scored ellipse : {}, ground-truth ellipse : {}'.format(name.upper(), s['map_iou_pred_' + name], s['map_iou_gt_' + name]))
    return ious, np.nanmedian(dists_pupil_seg), np.nanmedian(dists_iris_seg), float(np.mean(losses))


def main(argv=None):
    args = parse_args(argv)
    setting = _entry.load_setting(args.setting)
    rank, world = parallel.init()
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    collate = None
    if args.device_loader:
        from egne_amd import loader
        collate = loader.collate_raw
    if args.synthetic:
        testObj = loader.SyntheticRawEyes(args.synthetic) if args.device_loader else _entry.SyntheticEyes(args.synthetic)
        edge_net, model = _entry.seeded_networks(setting, args.model)
    else:
        from egne_amd.bdcn_new import BDCN
        from egne_amd.modelSummary import get_model
        if args.device_loader:
            testObj = loader.open_archive(args.raw_archive)
            collate = loader.collate_for(testObj)
        else:
            with open(os.path.join(args.path2data, 'baseline', 'cond_' + args.curObj + '.pkl'), 'rb') as f:
                _, _, testObj = pickle.load(f)                     # test.py:271-274
        edge_net = BDCN()
        edge_net.load_state_dict(torch.load('gen_00000016.pt', map_location='cpu')['a'])   # test.py:280-283
        model = get_model(args.model, setting)
        model.load_state_dict(torch.load(args.loadfile, map_location='cpu')['state_dict'], strict=False)
    _, samp = parallel.samplers(testObj, testObj, rank, world)
    loader = DataLoader(testObj, batch_size=args.batchsize, shuffle=False, sampler=samp, num_workers=args.workers, drop_last=True,
                        collate_fn=collate)
    edge_net, model = edge_net.to(device).eval(), model.to(device).to(args.prec)
    return calc_acc(args, loader, model, edge_net, device)


if __name__ == '__main__':
    main()
