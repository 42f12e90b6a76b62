"""The loss of encoder training (the reference's pSp/training/coach_new.py:285-320 calc_loss with pSp/criteria/w_norm.py): the weighted
sum of the image losses between a real image and its inversion, and the norm of the predicted codes.

    crit = EncoderLoss(id_loss=IDLoss('model_ir_se50.pth'), lpips_loss=AlexLPIPSLoss('alexnet.pth', 'alex.pth'))
    loss, loss_dict, id_logs = crit(real, inversed, z_code, p_code)          # the reference's defaults: id 0.1, l2 1.0, lpips 0.8
    loss.backward()                                                          # reaches `inversed` (and the codes through w_norm)

The terms, their order and the keys of loss_dict are calc_loss's: loss_id / id_improve (id_loss.IDLoss), loss_l2 (F.mse_loss),
loss_lpips (lpips_alex.AlexLPIPSLoss), loss_lpips_crop and loss_l2_crop on the window [35:223, 32:220] of both images, loss_w_norm
(the z and p codes' mean norm over dims (1, 2), after subtracting the latent averages where start_from_latent_avg), and loss.  A term
whose lambda is not positive is not computed.  L2 and the norms are plain torch on the device; the identity and LPIPS terms run on the
gfx950 kernels with their hand-written backward passes.  As in calc_loss, the identity term ASSIGNS the running sum (it comes first).
"""
import torch
import torch.nn.functional as F

CROP = (35, 223, 32, 220)        # coach_new.py:303, :307: rows 35:223, columns 32:220


def _scalar(v):
    """float(v) of a tensor that may carry a graph, or of a number"""
    return float(v.detach()) if torch.is_tensor(v) else float(v)


def w_norm(latent, latent_avg=None, start_from_latent_avg=False):
    """pSp/criteria/w_norm.py:11-14 WNormLoss.forward"""
    if start_from_latent_avg:
        if latent_avg is None:
            raise ValueError('EncoderLoss: start_from_latent_avg needs the latent averages (z_latent_avg, p_latent_avg)')
        latent = latent - latent_avg
    return torch.sum(latent.norm(2, dim=(1, 2))) / latent.shape[0]


class EncoderLoss(torch.nn.Module):
    def __init__(self, id_loss=None, lpips_loss=None, id_lambda=0.1, l2_lambda=1.0, lpips_lambda=0.8, lpips_lambda_crop=0, l2_lambda_crop=0,
                 w_norm_lambda=0, start_from_latent_avg=False):
        super().__init__()
        if id_lambda > 0 and id_loss is None:
            raise ValueError(f'EncoderLoss: id_lambda = {id_lambda} needs id_loss (transeditor_amd.id_loss.IDLoss)')
        if (lpips_lambda > 0 or lpips_lambda_crop > 0) and lpips_loss is None:
            name, v = ('lpips_lambda', lpips_lambda) if lpips_lambda > 0 else ('lpips_lambda_crop', lpips_lambda_crop)
            raise ValueError(f'EncoderLoss: {name} = {v} needs lpips_loss (transeditor_amd.lpips_alex.AlexLPIPSLoss)')
        self.id_loss, self.lpips_loss = id_loss, lpips_loss
        self.id_lambda, self.l2_lambda, self.lpips_lambda = id_lambda, l2_lambda, lpips_lambda
        self.lpips_lambda_crop, self.l2_lambda_crop, self.w_norm_lambda = lpips_lambda_crop, l2_lambda_crop, w_norm_lambda
        self.start_from_latent_avg = start_from_latent_avg

    def forward(self, real, inversed, z_code, p_code, z_latent_avg=None, p_latent_avg=None):
        """-> (loss, loss_dict, id_logs) of calc_loss(real_img, inversed_img, z_code, p_code)"""
        loss_dict, loss, id_logs = {}, 0.0, None
        y0, y1, x0, x1 = CROP
        if self.id_lambda > 0:
            loss_id, sim_improvement, id_logs = self.id_loss(inversed, real, real)
            loss_dict['loss_id'] = _scalar(loss_id)
            loss_dict['id_improve'] = _scalar(sim_improvement)
            loss = loss_id * self.id_lambda
        if self.l2_lambda > 0:
            loss_l2 = F.mse_loss(inversed, real)
            loss_dict['loss_l2'] = _scalar(loss_l2)
            loss = loss + loss_l2 * self.l2_lambda
        if self.lpips_lambda > 0:
            loss_lpips = self.lpips_loss(inversed, real)
            loss_dict['loss_lpips'] = _scalar(loss_lpips)
            loss = loss + loss_lpips * self.lpips_lambda
        if self.lpips_lambda_crop > 0:
            loss_lpips_crop = self.lpips_loss(inversed[:, :, y0:y1, x0:x1], real[:, :, y0:y1, x0:x1])
            loss_dict['loss_lpips_crop'] = _scalar(loss_lpips_crop)
            loss = loss + loss_lpips_crop * self.lpips_lambda_crop
        if self.l2_lambda_crop > 0:
            loss_l2_crop = F.mse_loss(inversed[:, :, y0:y1, x0:x1], real[:, :, y0:y1, x0:x1])
            loss_dict['loss_l2_crop'] = _scalar(loss_l2_crop)
            loss = loss + loss_l2_crop * self.l2_lambda_crop
        if self.w_norm_lambda > 0:
            loss_p_norm = w_norm(p_code, p_latent_avg, self.start_from_latent_avg)
            loss_z_norm = w_norm(z_code, z_latent_avg, self.start_from_latent_avg)
            loss_dict['loss_w_norm'] = _scalar(loss_p_norm) + _scalar(loss_z_norm)
            loss = loss + (loss_z_norm + loss_p_norm) * self.w_norm_lambda
        loss_dict['loss'] = _scalar(loss)
        return loss, loss_dict, id_logs
