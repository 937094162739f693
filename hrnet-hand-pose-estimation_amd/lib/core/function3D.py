"""Per-batch training / validation loops of the 3-D loss on MHP_mv batches (reference lib/core/function3D.py
train_helper / val_helper with AlgebraicTriangulationNet, lib/models/triangulation.py, and Joints3DMSELoss; the
recorder :505-628). The 2-D backbone is trained end to end on the error of the triangulated joints:

    model(imgs)[0]                                   (B*V, K, H, W) heat maps, slot b * V + v
    get_final_preds(hm, True)                        (B*V, K, 2) heat-map pixels, differentiable (expectation)
    proj = intrinsic[:, None] @ extrinsic            (B, V, 3, 4) float64
    triangulate_batch_of_points(proj, pred.view(B, V, K, 2), to_frame=hm_inverse)     (B, K, 3), ONE launch,
                                                     differentiable (utils/multiview.py, hrnet_triangulate_bwd)
    Joints3DMSELoss(X, pose3d_gt) * LOSS.POSE3D_LOSS_FACTOR
    + HeatmapLoss / JointsMSELoss (with visibility) on the heat-map-pixel predictions when their flags are on

This is the lifting tools/evaluate_3D.py evaluates, so the loss is the quantity that tool reports. The loops keep
core/function.py's conventions: running sums stay on the device and are read every PRINT_FREQ steps, the log line has
the same layout with the reference's label `Pose3DLoss` and scalar `train_loss/pose3d_loss`, `debug` stops an epoch
after 5 iterations. `validate` also reports the mean 3-D end-point error in mm (`EPE3D`, `val/epe3d`).

Deviations from the reference, deliberate:
- every parameter trains; the reference freezes the backbone below stage4;
- the points reach the frames through each image's `hm_inverse`, not through 640/64 and 480/64 (which does not
  invert the reader's crop);
- there is no confidence head: every view has weight 1 (MODEL.ALG_CONFIDENCES is refused by tools/train3D.py).
A separate module because core/function.py is the 2-D path and refuses a `pose3d_loss` criterion.
"""
import time

import torch

from utils.heatmap_decoding import get_final_preds
from utils.multiview import triangulate_batch_of_points

debug = False

DATASETS = ('MHP_mv',)

# (loss-dict key, LOSS flag, log label, LOSS factor)
_LOSS_NAMES = (('pose3d_loss', 'WITH_POSE3D_LOSS', 'Pose3DLoss', 'POSE3D_LOSS_FACTOR'),
               ('heatmap_loss', 'WITH_HEATMAP_LOSS', 'HeatmapLoss', 'HEATMAP_LOSS_FACTOR'),
               ('pose2d_loss', 'WITH_POSE2D_LOSS', 'Pose2DLoss', 'POSE2D_LOSS_FACTOR'))


class AverageMeter3D(object):
    """Running sums of the loss terms of the 3-D step and of the 3-D end-point error; `computeLosses` builds the total
    the step back-propagates. `criterion` maps 'pose3d_loss' (required) and optionally 'heatmap_loss' / 'pose2d_loss'
    to callables; the sums are whatever those return, detached - device tensors on the training path, read (one sync)
    only by the properties and computeAvgLosses."""

    def __init__(self, config, criterion):
        if 'pose3d_loss' not in criterion:
            raise ValueError("AverageMeter3D: the criterion dict has no 'pose3d_loss'")
        self.config = config
        self.criterion = criterion
        self._sums = {'total_loss': 0., 'epe3d': 0.}
        for key, _flag, _label, _factor in _LOSS_NAMES:
            if key in criterion:
                self._sums[key] = 0.
        self.n = 0

    def _read(self, key):
        v = self._sums.get(key)
        return None if v is None else (float(v.item()) if hasattr(v, 'item') else float(v))

    total_loss = property(lambda self: self._read('total_loss'))
    pose3d_loss = property(lambda self: self._read('pose3d_loss'))
    heatmap_loss = property(lambda self: self._read('heatmap_loss'))
    pose2d_loss = property(lambda self: self._read('pose2d_loss'))
    epe3d = property(lambda self: self._read('epe3d'))

    def computeAvgLosses(self):
        """{'total_loss', the enabled terms, 'epe3d'}: sums over the calls divided by their number; also avg_<key>"""
        n = max(self.n, 1)
        out = {}
        for key in self._sums:
            out[key] = self._read(key) / n
            setattr(self, 'avg_' + key, out[key])
        return out

    def computeLosses(self, pose3d_pred, pose3d_gt, heatmaps_pred=None, heatmaps_gt=None, pose2d_pred=None,
                      pose2d_gt=None, visibility=None, n=1):
        self.n += n
        L = self.config.LOSS
        out = dict.fromkeys(('pose3d_loss', 'heatmap_loss', 'pose2d_loss'))
        out['pose3d_loss'] = self.criterion['pose3d_loss'](pose3d_pred, pose3d_gt)
        if 'heatmap_loss' in self.criterion:
            out['heatmap_loss'] = self.criterion['heatmap_loss'](heatmaps_pred, heatmaps_gt)
        if 'pose2d_loss' in self.criterion:
            out['pose2d_loss'] = self.criterion['pose2d_loss'](pose2d_pred[:, :, 0:2], pose2d_gt[:, :, 0:2],
                                                               visibility=visibility)
        total = 0
        for key, _flag, _label, factor in _LOSS_NAMES:
            if out[key] is not None:
                self._sums[key] = self._sums[key] + out[key].detach()
                total = total + getattr(L, factor) * out[key]
        # mean over batch and joints of the 3-D distance, in the unit of the annotations (mm on MHP)
        epe = (pose3d_pred.detach().float() - pose3d_gt.detach().float()).norm(dim=-1).mean()
        self._sums['epe3d'] = self._sums['epe3d'] + epe
        self._sums['total_loss'] = self._sums['total_loss'] + total.detach()
        out['total_loss'] = total
        out['epe3d'] = epe
        return out


def _to_device(t, device):
    return t.cuda(device, non_blocking=True) if device is not None else t.cuda(non_blocking=True)


def lift(ret, model, device=None):
    """one MHP_mv batch through the model, the decode and the triangulation -> (heat maps (B*V, K, H, W), heat-map
    pixel predictions (B*V, K, 2), 3-D joints (B, K, 3)); differentiable when gradients are enabled"""
    imgs = _to_device(ret['imgs'], device)                         # (B*V, 3, H, W), slot b * V + v
    extrinsic = _to_device(ret['extrinsic_matrices'], device)
    V = extrinsic.shape[1]
    B = imgs.shape[0] // V
    heatmaps = model(imgs)[0]                                      # (heatmaps, inter_feat, temperature)
    pred = get_final_preds(heatmaps, True)
    proj = _to_device(ret['intrinsic_matrix'], device)[:, None] @ extrinsic
    pose3d = triangulate_batch_of_points(proj, pred.view(B, V, pred.shape[1], 2),
                                         to_frame=_to_device(ret['hm_inverse'], device))
    return heatmaps, pred, pose3d


def _forward_and_losses(config, ret, model, recorder, device):
    heatmaps, pred, pose3d = lift(ret, model, device)
    kw = {}
    if config.LOSS.WITH_HEATMAP_LOSS:
        kw.update(heatmaps_pred=heatmaps, heatmaps_gt=_to_device(ret['heatmaps'], device))
    if config.LOSS.WITH_POSE2D_LOSS:
        vis = _to_device(ret['visibility'], device)
        kw.update(pose2d_pred=pred, pose2d_gt=_to_device(ret['pose2d'], device),
                  visibility=vis.reshape(vis.shape[0], -1))
    return ret['imgs'], recorder.computeLosses(pose3d, _to_device(ret['pose3d'], device).float(), **kw)


def _message(head, batch_time, nimg, loss_dict, recorder, with_epe):
    msg = head + 'Time {:.3f}s\tSpeed {:.1f} samples/s\tTotalLoss {:.5f} ({:.5f})'.format(
        batch_time, nimg / batch_time, loss_dict['total_loss'].item(), recorder.avg_total_loss)
    for key, _flag, label, _factor in _LOSS_NAMES:
        if loss_dict[key] is not None:
            msg += '\t{} {:.5f} ({:.5f})'.format(label, loss_dict[key].item(), getattr(recorder, 'avg_' + key))
    if with_epe:
        msg += '\tEPE3D {:.3f} ({:.3f}) mm'.format(loss_dict['epe3d'].item(), recorder.avg_epe3d)
    return msg


def train_helper(epoch, i, args, config, master, ret, model, optimizer, dataset_name, train_loader, writer_dict,
                 logger, output_dir, tb_log_dir, recorder=None, device=None):
    end = time.time()
    imgs, loss_dict = _forward_and_losses(config, ret, model, recorder, device)
    total_loss = loss_dict['total_loss']
    optimizer.zero_grad()
    total_loss.backward()
    sync = getattr(model, '_segment_hook', None)
    if sync is not None:
        sync.finish()              # gradient all-reduce issued during backward (hipnet.optim.GradSync)
    optimizer.step()
    batch_time = time.time() - end
    if i % config.PRINT_FREQ == 0 and master:
        recorder.computeAvgLosses()
        head = 'Dataset: {0} Epoch: [{1}][{2}/{3}]\t'.format(dataset_name, epoch, i, len(train_loader))
        logger.info(_message(head, batch_time, imgs.size(0), loss_dict, recorder, with_epe=False))
        writer = writer_dict['writer']
        if writer is not None:
            steps = writer_dict['train_global_steps']
            for key, _flag, _label, _factor in _LOSS_NAMES:
                if loss_dict[key] is not None:
                    writer.add_scalar('train_loss/' + key, loss_dict[key], steps)
            writer.add_scalar('train_loss/total_loss', total_loss, steps)
    writer_dict['train_global_steps'] += 1


def train(config, args, master, train_loader_dict, model, criterion, optimizer, epoch, output_dir, tb_log_dir,
          writer_dict, logger, device=None):
    recorder = AverageMeter3D(config, criterion)
    model.train()
    for dataset_name, train_loader in train_loader_dict.items():
        logger.info('Training on {} dataset [Batch size: {}]\n'.format(dataset_name, train_loader.batch_size))
        if dataset_name not in DATASETS:
            raise NotImplementedError('dataset branch {}: the 3-D loss trains on MHP_mv batches'.format(dataset_name))
        for i, ret in enumerate(train_loader):
            train_helper(epoch, i, args, config, master, ret, model, optimizer, dataset_name, train_loader,
                         writer_dict, logger, output_dir, tb_log_dir, recorder=recorder, device=device)
            if debug and i == 4:
                break
    recorder.computeAvgLosses()
    return recorder


def val_helper(i, config, args, master, ret, model, dataset_name, val_loader, recorder, logger, device=None):
    end = time.time()
    imgs, loss_dict = _forward_and_losses(config, ret, model, recorder, device)
    if master and i % config.PRINT_FREQ == 0:
        batch_time = time.time() - end
        recorder.computeAvgLosses()
        head = 'Dataset: {0} Test: [{1}/{2}]\t'.format(dataset_name, i, len(val_loader))
        logger.info(_message(head, batch_time, imgs.size(0), loss_dict, recorder, with_epe=True))


def validate(config, args, master, val_loader_dict, model, criterion, output_dir, tb_log_dir, writer_dict, logger,
             device=None):
    recorder = AverageMeter3D(config, criterion)
    writer = writer_dict['writer']
    model.eval()
    for dataset_name, val_loader in val_loader_dict.items():
        logger.info('Validating on {} dataset [Batch size: {}]\n'.format(dataset_name, val_loader.batch_size))
        if dataset_name not in DATASETS:
            raise NotImplementedError('dataset branch {}: the 3-D loss validates on MHP_mv batches'.format(
                dataset_name))
        with torch.no_grad():
            for i, ret in enumerate(val_loader):
                val_helper(i, config, args, master, ret, model, dataset_name, val_loader, recorder, logger,
                           device=device)
                if debug and i == 4:
                    break
        avg = recorder.computeAvgLosses()
        if master:
            logger.info('Dataset: {} mean 3-D end-point error {:.3f} mm over {} batches'.format(
                dataset_name, avg['epe3d'], recorder.n))
        steps = writer_dict['valid_global_steps']
        if master and writer is not None:
            for key, value in avg.items():
                writer.add_scalar('val/epe3d' if key == 'epe3d' else 'val_loss/' + key, value, steps)
        writer_dict['valid_global_steps'] = steps + 1
    return recorder
