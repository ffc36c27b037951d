// Box regression losses on one aligned (pred, target) pair of (x1, y1, x2, y2) boxes: IoULoss (-log and linear), DIoULoss
// and CIoULoss of radet/models/losses/iou_loss.py:11-34,101-213, forward value and the gradient w.r.t. pred.  Shared by
// the stand-alone element kernels (boxops.hip) and the fused head loss (loss.hip); GIoU keeps its own code in both.
//
// The arithmetic follows the reference's PyTorch expressions operation by operation (compiled with
// -ffp-contract=off), including where eps enters:
//   IoU loss : bbox_overlaps(is_aligned=True) with ITS eps (union = max(union, 1e-6)), then .clamp(min=eps)
//   DIoU/CIoU: union = ap + ag - overlap + eps, c2 = cw^2 + ch^2 + eps, CIoU h1 / h2 carry + eps
// and the gradient is the case analysis autograd makes over those expressions: max / min ties split 1/2 - 1/2,
// clamp(min=..) passes the gradient at equality, torch.max(union, eps) splits it at equality.  CIoU's penalty
// v^2 / (1 - iou + v) is differentiated through v AND iou (this reference detaches no alpha).
#pragma once
#include "../../include/radet_hip.h"

#define BOX_OVERLAPS_EPS 1e-6f     // bbox_overlaps' own default eps (iou2d_calculator.py:72)
#define CIOU_FACTOR 0.40528473456935108578f     // 4 / pi^2

struct Box4 { float x1, y1, x2, y2; };

__device__ __forceinline__ float bl_gt(float a, float b) { return a > b ? 1.f : (a == b ? 0.5f : 0.f); }  // d max(a,b)/da
__device__ __forceinline__ float bl_lt(float a, float b) { return a < b ? 1.f : (a == b ? 0.5f : 0.f); }  // d min(a,b)/da
__device__ __forceinline__ float bl_ge0(float a) { return a >= 0.f ? 1.f : 0.f; }                         // d clamp(a, min=0)/da

// BWD == false: returns the loss, grad untouched.  BWD == true: returns the loss and writes g * d loss / d (px1, py1,
// px2, py2) to *grad (g = the upstream gradient of this element's loss).
template <int KIND, bool BWD>
__device__ __forceinline__ float box_loss_pair(const Box4 p, const Box4 t, float eps, float g, float4* grad) {
    static_assert(KIND == RADET_BOX_LOSS_IOU || KIND == RADET_BOX_LOSS_IOU_LINEAR || KIND == RADET_BOX_LOSS_DIOU ||
                  KIND == RADET_BOX_LOSS_CIOU, "GIoU has its own kernels");
    const float ltx = fmaxf(p.x1, t.x1), lty = fmaxf(p.y1, t.y1), rbx = fminf(p.x2, t.x2), rby = fminf(p.y2, t.y2);
    const float dw = rbx - ltx, dh = rby - lty;
    const float iw = fmaxf(dw, 0.f), ih = fmaxf(dh, 0.f);
    const float I = iw * ih;
    const float pw_ = p.x2 - p.x1, ph_ = p.y2 - p.y1;
    const float ap = pw_ * ph_, ag = (t.x2 - t.x1) * (t.y2 - t.y1);
    float loss;
    float g_I, g_ap;                                   // gradients w.r.t. overlap and pred area
    float gx1 = 0.f, gy1 = 0.f, gx2 = 0.f, gy2 = 0.f;   // everything that does not flow through I / ap
    if (KIND == RADET_BOX_LOSS_IOU || KIND == RADET_BOX_LOSS_IOU_LINEAR) {
        const float Uraw = (ap + ag) - I;
        const float U = fmaxf(Uraw, BOX_OVERLAPS_EPS);
        const float iou = I / U;
        const float c = fmaxf(iou, eps);
        loss = KIND == RADET_BOX_LOSS_IOU ? -logf(c) : 1.f - c;
        if (!BWD) return loss;
        const float g_c = KIND == RADET_BOX_LOSS_IOU ? -g / c : -g;
        const float g_iou = iou >= eps ? g_c : 0.f;
        const float g_Uraw = (-g_iou * I / (U * U)) * bl_gt(Uraw, BOX_OVERLAPS_EPS);
        g_I = g_iou / U - g_Uraw;
        g_ap = g_Uraw;
    } else {
        const float U = ((ap + ag) - I) + eps;
        const float iou = I / U;
        const float ex1 = fminf(p.x1, t.x1), ey1 = fminf(p.y1, t.y1), ex2 = fmaxf(p.x2, t.x2), ey2 = fmaxf(p.y2, t.y2);
        const float dew = ex2 - ex1, deh = ey2 - ey1;
        const float cw = fmaxf(dew, 0.f), ch = fmaxf(deh, 0.f);
        const float c2 = (cw * cw + ch * ch) + eps;
        const float ddx = (t.x1 + t.x2) - (p.x1 + p.x2), ddy = (t.y1 + t.y2) - (p.y1 + p.y2);
        const float rho2 = ddx * ddx / 4.f + ddy * ddy / 4.f;
        float v = 0.f, D = 1.f, pen = 0.f, w1 = 0.f, h1 = 1.f, q1 = 0.f, da = 0.f;
        if (KIND == RADET_BOX_LOSS_CIOU) {
            w1 = pw_;
            h1 = ph_ + eps;
            const float w2 = t.x2 - t.x1, h2 = (t.y2 - t.y1) + eps;
            q1 = w1 / h1;
            da = atanf(w2 / h2) - atanf(q1);
            v = CIOU_FACTOR * (da * da);
            D = (1.f - iou) + v;
            pen = v * v / D;
            loss = 1.f - (iou - (rho2 / c2 + pen));
        } else {
            loss = 1.f - (iou - rho2 / c2);
        }
        if (!BWD) return loss;
        float g_iou = -g;
        if (KIND == RADET_BOX_LOSS_CIOU) {
            const float r = v / D;                     // d pen / d v = 2 v / D - v^2 / D^2, d pen / d iou = v^2 / D^2
            g_iou += g * r * r;
            const float g_v = g * (2.f * r - r * r);
            const float g_q1 = -(g_v * CIOU_FACTOR * 2.f * da) / (1.f + q1 * q1);
            const float g_w1 = g_q1 / h1, g_h1 = -g_q1 * w1 / (h1 * h1);
            gx1 -= g_w1; gx2 += g_w1; gy1 -= g_h1; gy2 += g_h1;
        }
        const float g_U = -g_iou * I / (U * U);
        g_I = g_iou / U - g_U;
        g_ap = g_U;
        const float g_c2 = -g * rho2 / (c2 * c2);
        const float g_dew = g_c2 * 2.f * cw * bl_ge0(dew), g_deh = g_c2 * 2.f * ch * bl_ge0(deh);
        const float g_ddx = (g / c2) * ddx * 0.5f, g_ddy = (g / c2) * ddy * 0.5f;
        gx1 += -g_dew * bl_lt(p.x1, t.x1) - g_ddx;
        gy1 += -g_deh * bl_lt(p.y1, t.y1) - g_ddy;
        gx2 += g_dew * bl_gt(p.x2, t.x2) - g_ddx;
        gy2 += g_deh * bl_gt(p.y2, t.y2) - g_ddy;
    }
    const float g_dw = g_I * ih * bl_ge0(dw), g_dh = g_I * iw * bl_ge0(dh);
    grad->x = gx1 - g_dw * bl_gt(p.x1, t.x1) - g_ap * ph_;
    grad->y = gy1 - g_dh * bl_gt(p.y1, t.y1) - g_ap * pw_;
    grad->z = gx2 + g_dw * bl_lt(p.x2, t.x2) + g_ap * ph_;
    grad->w = gy2 + g_dh * bl_lt(p.y2, t.y2) + g_ap * pw_;
    return loss;
}
