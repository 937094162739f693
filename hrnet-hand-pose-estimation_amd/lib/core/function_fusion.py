"""Per-batch training / validation loops of the cross-view fusion model (MODEL.NAME multiview_pose_hrnet) on MHP_mv
batches: the `'MHP_mv' == dataset_name` branch of reference lib/core/function.py:195-276, with the conventions of
core/function3D.py (running sums stay on the device and are read every PRINT_FREQ steps).

    fused, single = model(imgs.view(B, V, 3, H, W))          models/multiview_pose_hrnet.py, each (B * V, K, h, w)
    heatmaps_pred = cat(single, fused); pose2d_pred = cat(decode(single), decode(fused))
    the targets, repeated twice                              (:212-216)
    HEATMAP_LOSS_FACTOR * HeatmapLoss + POSE2D_LOSS_FACTOR * JointsMSELoss (with visibility), per their LOSS flags

The log line has the reference's layout and labels (`TotalLoss`, `HeatmapLoss`, `Pose2DLoss`; scalars
`train_loss/heatmap_loss`, `train_loss/pose2d_loss`, `train_loss/total_loss`). `validate` reports the mean 2-D end-point
error in heat-map pixels over the visible joints, of the single-view maps and of the fused maps separately (`EPE2D single`,
`EPE2D fused`; `val/epe2d_single`, `val/epe2d_fused`), which is what the fusion layer is there to improve.

Rows are in slot order b * V + v on both sides, predictions and targets (the reader's order): see the module docstring
of models/multiview_pose_hrnet.py for why the reference's view-major concatenation is not reproduced.
"""
import time

import torch

from core.function3D import _to_device
import core.function3D as _f3d
from utils.heatmap_decoding import get_final_preds

debug = False

DATASETS = ('MHP_mv',)

# (loss-dict key, LOSS flag, log label, LOSS factor)
_LOSS_NAMES = (('heatmap_loss', 'WITH_HEATMAP_LOSS', 'HeatmapLoss', 'HEATMAP_LOSS_FACTOR'),
               ('pose2d_loss', 'WITH_POSE2D_LOSS', 'Pose2DLoss', 'POSE2D_LOSS_FACTOR'))
_EPES = ('epe2d_single', 'epe2d_fused')


class AverageMeterFusion(object):
    """Running sums of the loss terms of the fusion step and of the two 2-D end-point errors. `criterion` maps
    'heatmap_loss' and / or 'pose2d_loss' to callables; the sums are device tensors, read (one sync) only by
    computeAvgLosses and the avg_* attributes it sets."""

    def __init__(self, config, criterion):
        if not any(key in criterion for key, _f, _l, _c in _LOSS_NAMES):
            raise ValueError("AverageMeterFusion: the criterion dict has neither 'heatmap_loss' nor 'pose2d_loss'")
        self.config = config
        self.criterion = criterion
        self._sums = dict.fromkeys(('total_loss',) + _EPES, 0.)
        for key, _flag, _label, _factor in _LOSS_NAMES:
            if key in criterion:
                self._sums[key] = 0.
        self.n = 0

    def computeAvgLosses(self):
        n = max(self.n, 1)
        out = {}
        for key, v in self._sums.items():
            out[key] = (float(v.item()) if hasattr(v, 'item') else float(v)) / n
            setattr(self, 'avg_' + key, out[key])
        return out

    def computeLosses(self, heatmaps_pred, heatmaps_gt, pose2d_pred, pose2d_gt, visibility, n=1):
        """predictions: the concatenation [single; fused] (2 * B * V rows); targets: already repeated twice"""
        self.n += n
        L = self.config.LOSS
        out = dict.fromkeys(k for k, _f, _l, _c in _LOSS_NAMES)
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
        # mean distance over the visible joints, in heat-map pixels, of each half of the rows
        half = pose2d_pred.shape[0] // 2
        d = (pose2d_pred.detach()[:, :, 0:2].float() - pose2d_gt[:, :, 0:2].float()).norm(dim=-1)
        vis = visibility.float()
        for name, rows in zip(_EPES, (slice(0, half), slice(half, None))):
            out[name] = (d[rows] * vis[rows]).sum() / vis[rows].sum().clamp_min(1.0)
            self._sums[name] = self._sums[name] + out[name]
        self._sums['total_loss'] = self._sums['total_loss'] + total.detach()
        out['total_loss'] = total
        return out


def run_model(ret, model, device=None):
    """one MHP_mv batch through the model -> (fused, single), each (B * V, K, h, w); differentiable when gradients are
    enabled"""
    imgs = _to_device(ret['imgs'], device)                         # (B*V, 3, H, W), slot b * V + v
    V = ret['extrinsic_matrices'].shape[1]
    return model(imgs.view(imgs.shape[0] // V, V, *imgs.shape[1:]))


def _forward_and_losses(config, ret, model, recorder, device):
    fused, single = run_model(ret, model, device)
    softmax = config.MODEL.HEATMAP_SOFTMAX
    heatmaps_pred = torch.cat((single, fused), dim=0)
    pose2d_pred = torch.cat((get_final_preds(single, use_softmax=softmax), get_final_preds(fused, use_softmax=softmax)),
                            dim=0)
    heatmaps_gt = None
    if config.LOSS.WITH_HEATMAP_LOSS:
        heatmaps_gt = _to_device(ret['heatmaps'], device).repeat((2, 1, 1, 1))
    pose2d_gt = _to_device(ret['pose2d'], device).repeat((2, 1, 1))
    vis = _to_device(ret['visibility'], device)
    vis = vis.reshape(vis.shape[0], -1).repeat((2, 1))
    return ret['imgs'], recorder.computeLosses(heatmaps_pred, heatmaps_gt, pose2d_pred, pose2d_gt, vis)


def _message(head, batch_time, nimg, loss_dict, recorder, with_epe):
    msg = head + 'Time {:.3f}s\tSpeed {:.1f} samples/s\tTotalLoss {:.5f} ({:.5f})'.format(
        batch_time, nimg / batch_time, loss_dict['total_loss'].item(), recorder.avg_total_loss)
    for key, _flag, label, _factor in _LOSS_NAMES:
        if loss_dict[key] is not None:
            msg += '\t{} {:.5f} ({:.5f})'.format(label, loss_dict[key].item(), getattr(recorder, 'avg_' + key))
    if with_epe:
        msg += '\tEPE2D single {:.3f} ({:.3f}) px\tEPE2D fused {:.3f} ({:.3f}) px'.format(
            loss_dict['epe2d_single'].item(), recorder.avg_epe2d_single, loss_dict['epe2d_fused'].item(),
            recorder.avg_epe2d_fused)
    return msg


def train_helper(epoch, i, args, config, master, ret, model, optimizer, dataset_name, train_loader, writer_dict,
                 logger, output_dir, tb_log_dir, recorder=None, device=None):
    end = time.time()
    imgs, loss_dict = _forward_and_losses(config, ret, model, recorder, device)
    total_loss = loss_dict['total_loss']
    optimizer.zero_grad()
    total_loss.backward()
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
    recorder = AverageMeterFusion(config, criterion)
    model.train()
    for dataset_name, train_loader in train_loader_dict.items():
        logger.info('Training on {} dataset [Batch size: {}]\n'.format(dataset_name, train_loader.batch_size))
        if dataset_name not in DATASETS:
            raise NotImplementedError('dataset branch {}: the fusion model trains on MHP_mv batches'.format(
                dataset_name))
        for i, ret in enumerate(train_loader):
            train_helper(epoch, i, args, config, master, ret, model, optimizer, dataset_name, train_loader,
                         writer_dict, logger, output_dir, tb_log_dir, recorder=recorder, device=device)
            if (debug or _f3d.debug) and i == 4:
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
    recorder = AverageMeterFusion(config, criterion)
    writer = writer_dict['writer']
    model.eval()
    for dataset_name, val_loader in val_loader_dict.items():
        logger.info('Validating on {} dataset [Batch size: {}]\n'.format(dataset_name, val_loader.batch_size))
        if dataset_name not in DATASETS:
            raise NotImplementedError('dataset branch {}: the fusion model validates on MHP_mv batches'.format(
                dataset_name))
        with torch.no_grad():
            for i, ret in enumerate(val_loader):
                val_helper(i, config, args, master, ret, model, dataset_name, val_loader, recorder, logger,
                           device=device)
                if (debug or _f3d.debug) and i == 4:
                    break
        avg = recorder.computeAvgLosses()
        if master:
            logger.info('Dataset: {} mean 2-D end-point error: single {:.3f} px, fused {:.3f} px over {} batches'.format(
                dataset_name, avg['epe2d_single'], avg['epe2d_fused'], recorder.n))
        steps = writer_dict['valid_global_steps']
        if master and writer is not None:
            for key, value in avg.items():
                writer.add_scalar('val/' + key if key in _EPES else 'val_loss/' + key, value, steps)
        writer_dict['valid_global_steps'] = steps + 1
    return recorder
