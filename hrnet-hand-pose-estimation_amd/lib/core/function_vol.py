"""Per-batch training / validation loops of the volumetric model on MHP_mv batches (the `"vol" in model_type` branch of
reference lib/core/function3D.py:78-189, the recorder :505-628), with the conventions of core/function3D.py:

    proj = A K [R|t]                                  (B, V, 3, 4): world -> heat-map pixels, per image
    model(imgs.view(B, V, 3, H, W), proj)             models/triangulation.py, VolumetricTriangulationNet
    POSE3D_LOSS_FACTOR * Joints3DMSELoss(vol_keypoints_3d, pose3d_gt)
    + VOLUMETRIC_LOSS_FACTOR * VolumetricCELoss(coord_volumes, volumes, pose3d_gt, ones)     when WITH_VOLUMETRIC_CE_LOSS
    + HeatmapLoss / JointsMSELoss (with visibility) on the heat maps and their decode when their flags are on

Running sums stay on the device and are read every PRINT_FREQ steps; the log line has function3D's layout with the
reference's labels `Pose3DLoss` and `VolumetricCELoss` and the scalars `train_loss/pose3d_loss` and
`train_loss/volumetric_ce_loss`; `validate` reports the mean 3-D end-point error in mm (`EPE3D`, `val/epe3d`).

MHP_CPM_mv batches (MODEL.NAME vol_CPM) carry `centermaps`, which go to the model between the images and the
projection matrices, and their own `heatmaps` target with k + 1 channels (the background first), which the heat-map term
takes as it is; the loss composition is the same.

Deviation from the reference, deliberate and the one core/function3D.py documents: A is the 3x3 frame-to-heat-map map
obtained by inverting the reader's `hm_inverse` of each image. The reference's update_after_resize scales the
intrinsics by 64/640 and 64/480, which does not invert the reader's crop.
"""
import time

import torch

from core.function3D import AverageMeter3D, _to_device
import core.function3D as _f3d

debug = False

DATASETS = ('MHP_mv', 'MHP_CPM_mv')

# (loss-dict key, LOSS flag, log label, LOSS factor)
_LOSS_NAMES = (('pose3d_loss', 'WITH_POSE3D_LOSS', 'Pose3DLoss', 'POSE3D_LOSS_FACTOR'),
               ('volumetric_ce_loss', 'WITH_VOLUMETRIC_CE_LOSS', 'VolumetricCELoss', 'VOLUMETRIC_LOSS_FACTOR'),
               ('heatmap_loss', 'WITH_HEATMAP_LOSS', 'HeatmapLoss', 'HEATMAP_LOSS_FACTOR'),
               ('pose2d_loss', 'WITH_POSE2D_LOSS', 'Pose2DLoss', 'POSE2D_LOSS_FACTOR'))


def heatmap_projections(intrinsic, extrinsic, hm_inverse):
    """intrinsic (B, 3, 3), extrinsic (B, V, 3, 4), hm_inverse (B * V, 2, 3) -> (B, V, 3, 4) float64 projection
    matrices A K [R|t] from world coordinates to heat-map pixels; A = [hm_inverse; 0 0 1]^-1 in closed form (the map is
    affine), on the tensors' device"""
    B, V = extrinsic.shape[:2]
    M = hm_inverse.to(torch.float64).reshape(B, V, 2, 3)
    a, b, tx = M[..., 0, 0], M[..., 0, 1], M[..., 0, 2]
    c, d, ty = M[..., 1, 0], M[..., 1, 1], M[..., 1, 2]
    det = a * d - b * c
    A = torch.zeros((B, V, 3, 3), dtype=torch.float64, device=M.device)
    A[..., 0, 0], A[..., 0, 1], A[..., 0, 2] = d / det, -b / det, (b * ty - d * tx) / det
    A[..., 1, 0], A[..., 1, 1], A[..., 1, 2] = -c / det, a / det, (c * tx - a * ty) / det
    A[..., 2, 2] = 1.0
    return A @ (intrinsic.to(torch.float64)[:, None] @ extrinsic.to(torch.float64))


class AverageMeterVol(AverageMeter3D):
    """core.function3D.AverageMeter3D with the volumetric cross-entropy term: `criterion` maps 'pose3d_loss'
    (required) and optionally 'volumetric_ce_loss', 'heatmap_loss', 'pose2d_loss' to callables"""

    def __init__(self, config, criterion):
        super(AverageMeterVol, self).__init__(config, criterion)
        if 'volumetric_ce_loss' in criterion:
            self._sums['volumetric_ce_loss'] = 0.

    volumetric_ce_loss = property(lambda self: self._read('volumetric_ce_loss'))

    def computeLosses(self, pose3d_pred, pose3d_gt, coord_volumes=None, volumes=None, heatmaps_pred=None,
                      heatmaps_gt=None, pose2d_pred=None, pose2d_gt=None, visibility=None, n=1):
        self.n += n
        L = self.config.LOSS
        out = dict.fromkeys(k for k, _f, _l, _c in _LOSS_NAMES)
        out['pose3d_loss'] = self.criterion['pose3d_loss'](pose3d_pred, pose3d_gt)
        if 'volumetric_ce_loss' in self.criterion:
            validity = torch.ones(pose3d_gt.shape[:2] + (1,), dtype=torch.float32, device=pose3d_gt.device)
            out['volumetric_ce_loss'] = self.criterion['volumetric_ce_loss'](coord_volumes, volumes, pose3d_gt, validity)
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
        epe = (pose3d_pred.detach().float() - pose3d_gt.detach().float()).norm(dim=-1).mean()
        self._sums['epe3d'] = self._sums['epe3d'] + epe
        self._sums['total_loss'] = self._sums['total_loss'] + total.detach()
        out['total_loss'] = total
        out['epe3d'] = epe
        return out


def run_model(ret, model, device=None):
    """one MHP_mv or MHP_CPM_mv batch through the model -> its 7-tuple; differentiable when gradients are enabled"""
    imgs = _to_device(ret['imgs'], device)                         # (B*V, 3, H, W), slot b * V + v
    extrinsic = ret['extrinsic_matrices']
    B, V = extrinsic.shape[:2]
    proj = heatmap_projections(ret['intrinsic_matrix'], extrinsic, ret['hm_inverse'])
    imgs = imgs.view(B, V, *imgs.shape[1:])
    if 'centermaps' in ret:                                        # MHP_CPM_mv: the model on the CPM backbone
        cm = _to_device(ret['centermaps'], device).float()
        return model(imgs, cm.view(B, V, *cm.shape[1:]), _to_device(proj.float(), device))
    return model(imgs, _to_device(proj.float(), device))


def _forward_and_losses(config, ret, model, recorder, device):
    pose3d, pose2d_pred, heatmaps, volumes, _conf, coord_volumes, _base = run_model(ret, model, device)
    kw = {}
    if config.LOSS.WITH_VOLUMETRIC_CE_LOSS:
        kw.update(coord_volumes=coord_volumes, volumes=volumes)
    if config.LOSS.WITH_HEATMAP_LOSS:
        kw.update(heatmaps_pred=heatmaps.reshape(-1, *heatmaps.shape[2:]),
                  heatmaps_gt=_to_device(ret['heatmaps'], device))
    if config.LOSS.WITH_POSE2D_LOSS:
        vis = _to_device(ret['visibility'], device)
        kw.update(pose2d_pred=pose2d_pred.reshape(-1, *pose2d_pred.shape[2:]),
                  pose2d_gt=_to_device(ret['pose2d'], device), visibility=vis.reshape(vis.shape[0], -1))
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
    recorder = AverageMeterVol(config, criterion)
    model.train()
    for dataset_name, train_loader in train_loader_dict.items():
        logger.info('Training on {} dataset [Batch size: {}]\n'.format(dataset_name, train_loader.batch_size))
        if dataset_name not in DATASETS:
            raise NotImplementedError('dataset branch {}: the volumetric model trains on MHP_mv batches'.format(
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
    recorder = AverageMeterVol(config, criterion)
    writer = writer_dict['writer']
    model.eval()
    for dataset_name, val_loader in val_loader_dict.items():
        logger.info('Validating on {} dataset [Batch size: {}]\n'.format(dataset_name, val_loader.batch_size))
        if dataset_name not in DATASETS:
            raise NotImplementedError('dataset branch {}: the volumetric model validates on MHP_mv batches'.format(
                dataset_name))
        with torch.no_grad():
            for i, ret in enumerate(val_loader):
                val_helper(i, config, args, master, ret, model, dataset_name, val_loader, recorder, logger,
                           device=device)
                if (debug or _f3d.debug) and i == 4:
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
