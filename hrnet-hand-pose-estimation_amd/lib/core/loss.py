"""Loss modules of the hot path (reference lib/core/loss.py:15-50, 150-223) on HIP kernels.

HeatmapLoss    mean over (B,K) of the per-map sum of (pred-gt)^2 (mode 'l2') or |pred-gt| ('l1')
JointsMSELoss  visibility-weighted mean L2 norm of key-point errors (despite its name)
Joints3DMSELoss sum over batch and joints of the L2 norm of the 3-D error, over K (reference :137-148: a sum over the
               batch); f64 inside, fixed summation order
BoneLengthLoss sum over batch and j = 1..20 of (|gt[j]-gt[j-1]| - |pred[j]-pred[j-1]|)^2, over 20: a sum over the
               batch, and EVERY consecutive pair is a bone (5-4, 9-8, 13-12, 17-16 included - the reference's
               finger-base branch is never taken)
JointAngleLoss sum over batch and fingers (joints 4f..4f+4) of d^2 for each negative product d of neighbouring
               bone cross products (z components; the coplanarity rule is identically zero for 2-D poses)
VolumetricCELoss  the volumetric models' regulariser (reference :225-256): -log of the predicted volume at the voxel
               nearest the ground truth, validity-weighted, over the number of joints; the nearest-voxel search
               and the sum are one call (hrnet_volumetric_ce_loss), f64 inside, fixed summation order
structure_losses  what the training loop calls: both terms after scale_pose2d (relative to the wrist, divided by
               the wrist-to-joint-9 length, no epsilon) of pred and gt, ONE launch (hrnet_structure_loss) that also
               leaves d bone / d pred and d angle / d pred when pred requires grad; backward is one launch that
               combines them with the upstream gradients, nothing is recomputed

All are autograd Functions over the C ABI (hrnet_heatmap_loss_*, hrnet_joints_loss_*, hrnet_joints3d_loss_*,
hrnet_structure_loss*, hrnet_volumetric_ce_loss*);
inputs must be HIP tensors - there is no CPU path. The structure terms take B x 21 x 2 poses only: 3-D poses (a real
z, the reference's other use of the two classes) are refused.

Degenerate poses follow IEEE and the reference: a zero-length bone has no gradient (torch.norm backward is 0 at
the origin); pred[9] == pred[0] (zero scale) makes both losses and that sample's gradients NaN/inf. A freshly
initialised softmax model decodes every joint close to the map centre, so BoneLengthLoss / JointAngleLoss are meant
to be switched on from a trained checkpoint, as in the reference.
"""
import torch
import torch.nn as nn

from hipnet import _capi as C


def _dev_f32(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError('{}: expected a HIP-device tensor (no CPU path in this build)'.format(what))
    return t.contiguous().float()


class _HeatmapLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, mode):
        bk = pred.shape[0] * pred.shape[1] if pred.dim() == 4 else pred.shape[0]
        hw = pred.shape[-1] * pred.shape[-2]
        partial = torch.empty(bk, dtype=torch.float32, device=pred.device)
        loss = torch.empty(1, dtype=torch.float32, device=pred.device)
        C.call('hrnet_heatmap_loss_fwd', pred.data_ptr(), gt.data_ptr(), partial.data_ptr(), loss.data_ptr(), bk, hw,
               mode, C.stream_ptr())
        ctx.save_for_backward(pred, gt)
        ctx.mode, ctx.bk, ctx.hw = mode, bk, hw
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gout):
        pred, gt = ctx.saved_tensors
        dpred = torch.empty_like(pred)
        g = gout.contiguous().float().reshape(1)
        C.call('hrnet_heatmap_loss_bwd', pred.data_ptr(), gt.data_ptr(), g.data_ptr(), dpred.data_ptr(), ctx.bk, ctx.hw,
               ctx.mode, C.stream_ptr())
        return dpred, None, None


class HeatmapLoss(nn.Module):
    def __init__(self, mode='l2'):
        super().__init__()
        if mode not in ('l2', 'l1'):
            raise ValueError("HeatmapLoss mode must be 'l2' or 'l1'")
        self.mode = mode

    def forward(self, pred, gt):
        assert pred.size() == gt.size(), \
            'Heatmap loss error: prediced heatmaps have size {}, but the groundtruth has {}'.format(pred.shape, gt.shape)
        pred = _dev_f32(pred, 'HeatmapLoss')
        gt = _dev_f32(gt, 'HeatmapLoss').detach()
        return _HeatmapLossFn.apply(pred, gt, 0 if self.mode == 'l2' else 1)


class _JointsLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, vis):
        b, k = pred.shape[0], pred.shape[1]
        loss = torch.empty(1, dtype=torch.float32, device=pred.device)
        C.call('hrnet_joints_loss_fwd', pred.data_ptr(), gt.data_ptr(), C.ptr(vis), loss.data_ptr(), b, k,
               C.stream_ptr())
        ctx.save_for_backward(pred, gt, vis)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gout):
        pred, gt, vis = ctx.saved_tensors
        dpred = torch.empty_like(pred)
        g = gout.contiguous().float().reshape(1)
        C.call('hrnet_joints_loss_bwd', pred.data_ptr(), gt.data_ptr(), C.ptr(vis), g.data_ptr(), dpred.data_ptr(),
               pred.shape[0], pred.shape[1], C.stream_ptr())
        return dpred, None, None


class JointsMSELoss(nn.Module):
    """pose2D_pred, pose2D_gt: B x K x 2; visibility: B x K (optional)."""

    def forward(self, pose2D_pred, pose2D_gt, visibility=None):
        pred = _dev_f32(pose2D_pred, 'JointsMSELoss')
        gt = _dev_f32(pose2D_gt, 'JointsMSELoss').detach()
        if pred.dim() != 3 or pred.shape[2] != 2:
            raise ValueError('JointsMSELoss expects B x K x 2 key points')
        vis = None
        if visibility is not None:
            vis = _dev_f32(visibility.to(pred.device), 'JointsMSELoss').reshape(pred.shape[0], pred.shape[1]).detach()
        return _JointsLossFn.apply(pred, gt, vis)


class _Joints3DLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt):
        loss = torch.empty(1, dtype=torch.float32, device=pred.device)
        C.call('hrnet_joints3d_loss_fwd', pred.data_ptr(), gt.data_ptr(), loss.data_ptr(), pred.shape[0],
               pred.shape[1], C.stream_ptr())
        ctx.save_for_backward(pred, gt)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gout):
        pred, gt = ctx.saved_tensors
        dpred = torch.empty_like(pred)
        g = gout.contiguous().float().reshape(1)
        C.call('hrnet_joints3d_loss_bwd', pred.data_ptr(), gt.data_ptr(), g.data_ptr(), dpred.data_ptr(),
               pred.shape[0], pred.shape[1], C.stream_ptr())
        return dpred, None


class Joints3DMSELoss(nn.Module):
    """pose3d_pred, pose3d_gt: B x K x 3 -> sum_{b,k} ||gt - pred||_2 / K (a sum over the batch, as the reference)."""

    def forward(self, pose3d_pred, pose3d_gt):
        pred = _dev_f32(pose3d_pred, 'Joints3DMSELoss')
        gt = _dev_f32(pose3d_gt, 'Joints3DMSELoss').detach()
        if pred.dim() != 3 or pred.shape[2] != 3 or pred.shape != gt.shape:
            raise ValueError('Joints3DMSELoss expects two B x K x 3 poses, got {} and {}'.format(
                tuple(pred.shape), tuple(gt.shape)))
        return _Joints3DLossFn.apply(pred, gt)


class _VolumetricCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, coord, gt, validity):
        B, J, X, Y, Z = p.shape
        loss = torch.empty(1, dtype=torch.float32, device=p.device)
        idx = torch.empty((B, J), dtype=torch.int32, device=p.device)
        C.call('hrnet_volumetric_ce_loss', coord.data_ptr(), p.data_ptr(), gt.data_ptr(), validity.data_ptr(),
               loss.data_ptr(), idx.data_ptr(), B, J, X, Y, Z, C.stream_ptr())
        ctx.save_for_backward(p, validity, idx)
        ctx.mark_non_differentiable(idx)
        return loss.reshape(()), idx

    @staticmethod
    def backward(ctx, gout, _gidx):
        p, validity, idx = ctx.saved_tensors
        B, J, X, Y, Z = p.shape
        dp = torch.empty_like(p)
        g = gout.contiguous().float().reshape(1)
        C.call('hrnet_volumetric_ce_loss_bwd', p.data_ptr(), validity.data_ptr(), idx.data_ptr(), g.data_ptr(),
               dp.data_ptr(), B, J, X, Y, Z, C.stream_ptr())
        return dp, None, None, None


class VolumetricCELoss(nn.Module):
    """The volumetric cross-entropy regulariser (reference :225-256): per joint the voxel of the coordinate volume
    nearest the ground truth (f64 distances, the first of equals), then sum validity * -log(p[voxel] + 1e-6) over the
    number of joints, valid or not. coord_volumes_batch B x X x Y x Z x 3, volumes_batch_pred B x J x X x Y x Z (the
    second output of integrate_tensor_3d_with_coordinates), keypoints_gt B x J x 3, keypoints_binary_validity
    B x J x 1 as the reference indexes it (B x J is taken too). forward returns the loss, as the reference;
    loss_and_indices also returns the chosen flat voxel indices x*Y*Z + y*Z + z (B x J int32). No state is kept."""

    def forward(self, coord_volumes_batch, volumes_batch_pred, keypoints_gt, keypoints_binary_validity):
        return self.loss_and_indices(coord_volumes_batch, volumes_batch_pred, keypoints_gt,
                                     keypoints_binary_validity)[0]

    def loss_and_indices(self, coord_volumes_batch, volumes_batch_pred, keypoints_gt, keypoints_binary_validity):
        p = _dev_f32(volumes_batch_pred, 'VolumetricCELoss')
        if p.dim() != 5:
            raise ValueError('VolumetricCELoss expects B x J x X x Y x Z volumes, got {}'.format(tuple(p.shape)))
        B, J = p.shape[:2]
        coord = _dev_f32(coord_volumes_batch, 'VolumetricCELoss').detach()
        gt = _dev_f32(keypoints_gt, 'VolumetricCELoss').detach()
        validity = _dev_f32(keypoints_binary_validity, 'VolumetricCELoss').detach()
        if tuple(coord.shape) != (B,) + tuple(p.shape[2:]) + (3,) or tuple(gt.shape) != (B, J, 3) \
                or validity.numel() != B * J:
            raise ValueError('VolumetricCELoss: coord volumes {}, volumes {}, key points {}, validity {}'.format(
                tuple(coord.shape), tuple(p.shape), tuple(gt.shape), tuple(validity.shape)))
        return _VolumetricCEFn.apply(p, coord, gt, validity.reshape(B, J))


TERM_BONE, TERM_ANGLE = 1, 2


def _check_hand_pose(t, what, name, vis_column=False):
    """shape rules of the structure losses; they are checked for every argument before any device rule"""
    if not isinstance(t, torch.Tensor) or t.dim() != 3:
        raise ValueError('{}: {} must be a B x 21 x 2 tensor'.format(what, name))
    if t.shape[2] == 3 and not vis_column:
        raise ValueError('{}: {} has 3 columns - 3-D poses (and the coplanarity rule that goes with them) are out of '
                         'scope here, pass B x 21 x 2 image coordinates without a z column'.format(what, name))
    if t.shape[2] not in ((2, 3) if vis_column else (2,)):
        raise ValueError('{}: {} must be a B x 21 x 2 tensor, got {}'.format(what, name, tuple(t.shape)))
    if t.shape[1] != 21:
        raise ValueError('{}: {} has K = {} joints, the hand skeleton of these losses has 21'.format(
            what, name, t.shape[1]))
    if t.shape[0] < 1:
        raise ValueError('{}: empty batch'.format(what))


def _hand_pose(t, what):
    """B x 21 x 2 f32 on the device (a third visibility column of the ground truth is dropped)"""
    return _dev_f32(t[:, :, 0:2] if isinstance(t, torch.Tensor) else t, what)


def _structure_forward(pred, gt, terms, normalize, want_grad):
    """one hrnet_structure_loss launch -> (bone, angle, (dbone, dangle) or None); a term that is off is None, in
    the losses and in the pair of unit gradients [B, 21, 2]"""
    b = pred.shape[0]
    bone = torch.empty((), dtype=torch.float32, device=pred.device) if terms & TERM_BONE else None
    angle = torch.empty((), dtype=torch.float32, device=pred.device) if terms & TERM_ANGLE else None
    grads = None
    if want_grad:                                 # one allocation; a term that is off has no buffer
        buf = torch.empty((bin(terms).count('1'), b, 21, 2), dtype=torch.float32, device=pred.device)
        grads = (buf[0] if terms & TERM_BONE else None, buf[-1] if terms & TERM_ANGLE else None)
    C.call('hrnet_structure_loss', pred.data_ptr(), C.ptr(gt), C.ptr(bone), C.ptr(angle),
           C.ptr(grads[0]) if want_grad else None, C.ptr(grads[1]) if want_grad else None, b, 21,
           1 if normalize else 0, terms, C.stream_ptr())
    return bone, angle, grads


class _StructureLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, terms, normalize, want_grad):
        bone, angle, grads = _structure_forward(pred, gt, terms, normalize, want_grad)
        ctx.grads = grads
        ctx.set_materialize_grads(False)          # an unused term must not put 0 * NaN into the gradient
        return bone, angle

    @staticmethod
    def backward(ctx, g_bone, g_angle):
        grads = ctx.grads
        if grads is None or (g_bone is None and g_angle is None):
            return None, None, None, None, None
        if g_bone is None:
            dpred = torch.empty_like(grads[1])
        else:
            dpred = torch.empty_like(grads[0])
        gb = None if g_bone is None else g_bone.contiguous().float().reshape(1)
        ga = None if g_angle is None else g_angle.contiguous().float().reshape(1)
        C.call('hrnet_structure_loss_bwd', C.ptr(grads[0]), C.ptr(grads[1]), C.ptr(gb), C.ptr(ga),
               dpred.data_ptr(), dpred.shape[0], 21, C.stream_ptr())
        return dpred, None, None, None, None


def structure_losses(pose2d_pred, pose2d_gt=None, terms=TERM_BONE | TERM_ANGLE, normalize=True):
    """(bone_loss, jointangle_loss) of B x 21 x 2 poses in one launch; a term left out of `terms` is None.

    normalize: apply the reference's scale_pose2d to both poses first (what its training loop does). pose2d_gt may
    carry a third visibility column, which is ignored; it is needed for the bone term only."""
    if terms not in (TERM_BONE, TERM_ANGLE, TERM_BONE | TERM_ANGLE):
        raise ValueError('structure_losses: terms is TERM_BONE, TERM_ANGLE or both')
    _check_hand_pose(pose2d_pred, 'structure_losses', 'pose2d_pred')
    if terms & TERM_BONE:
        if pose2d_gt is None:
            raise ValueError('structure_losses: the bone-length term needs pose2d_gt')
        _check_hand_pose(pose2d_gt, 'structure_losses', 'pose2d_gt', vis_column=True)
        if pose2d_gt.shape[0] != pose2d_pred.shape[0]:
            raise ValueError('structure_losses: pose2d_pred and pose2d_gt differ in batch size')
    pred = _hand_pose(pose2d_pred, 'structure_losses')
    gt = _hand_pose(pose2d_gt, 'structure_losses').detach() if terms & TERM_BONE else None
    want_grad = torch.is_grad_enabled() and pred.requires_grad
    return _StructureLossFn.apply(pred, gt, terms, bool(normalize), want_grad)


class BoneLengthLoss(nn.Module):
    """pose_pred, pose_gt: B x 21 x 2, taken as given (no normalisation), as the reference module."""

    def forward(self, pose23d_pred, pose23d_gt):
        _check_hand_pose(pose23d_pred, 'BoneLengthLoss', 'pose_pred')
        _check_hand_pose(pose23d_gt, 'BoneLengthLoss', 'pose_gt')
        if pose23d_gt.shape[0] != pose23d_pred.shape[0]:
            raise ValueError('BoneLengthLoss: pose_pred and pose_gt differ in batch size')
        pred = _hand_pose(pose23d_pred, 'BoneLengthLoss')
        gt = _hand_pose(pose23d_gt, 'BoneLengthLoss').detach()
        want_grad = torch.is_grad_enabled() and pred.requires_grad
        return _StructureLossFn.apply(pred, gt, TERM_BONE, False, want_grad)[0]


class JointAngleLoss(nn.Module):
    """pose_pred: B x 21 x 2, taken as given. The reference pads 2-D poses with z = 0 for torch.cross; here they
    are passed without the padding."""

    def forward(self, pose23d_pred):
        _check_hand_pose(pose23d_pred, 'JointAngleLoss', 'pose_pred')
        pred = _hand_pose(pose23d_pred, 'JointAngleLoss')
        want_grad = torch.is_grad_enabled() and pred.requires_grad
        return _StructureLossFn.apply(pred, None, TERM_ANGLE, False, want_grad)[1]
