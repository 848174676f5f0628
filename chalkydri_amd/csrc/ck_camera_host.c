// Camera models, the half that needs no device: the parameter check every entry point shares and the one-thread twins
// of the unprojection kernels.  The arithmetic is ck_camera_math.h's, the same text the kernels compile, so the bytes are theirs.
#include "chalkydri_hip.h"
#include "ck_camera_math.h"

int ck_camera_check(const ck_camera_t *cam) {
    if (!cam) return CK_EINVAL;
    if (cam->model != CK_CAMERA_OPENCV5 && cam->model != CK_CAMERA_EUCM && cam->model != CK_CAMERA_UCM) return CK_EINVAL;
    double k[9];
    ckm_effective(cam->model, cam->k, k); // (UCM's k[5] is 1.0 from here on: what the slot holds is never looked at)
    for (int i = 0; i < 9; i++)
        if (!ckm_finite(k[i])) return CK_EINVAL;
    if (!(k[0] > 0.0) || !(k[1] > 0.0)) return CK_EINVAL;
    if (cam->model == CK_CAMERA_OPENCV5) return CK_OK;
    if (!(k[4] >= 0.0) || !(k[4] <= 1.0)) return CK_EINVAL;
    if (!(k[5] > 0.0)) return CK_EINVAL;
    if (k[6] != 0.0 || k[7] != 0.0 || k[8] != 0.0) return CK_EINVAL;
    return CK_OK;
}

int ck_camera_unproject_host(const ck_camera_t *cam, const double *px, int32_t n, double *bearings, uint8_t *ok) {
    const int rc = ck_camera_check(cam);
    if (rc != CK_OK) return rc;
    if (!px || !bearings || !ok || n < 0) return CK_EINVAL;
    double k[9];
    ckm_effective(cam->model, cam->k, k);
    for (int32_t i = 0; i < n; i++) {
        const int good = cam->model == CK_CAMERA_OPENCV5 ? ckm_opencv5_unproject(k, px[2 * i], px[2 * i + 1], bearings + 3 * (size_t)i)
                                                         : ckm_eucm_unproject(k, px[2 * i], px[2 * i + 1], bearings + 3 * (size_t)i);
        ok[i] = good ? 1 : 0;
    }
    return CK_OK;
}

int ck_camera_normalize_host(const ck_camera_t *cam, const double *px, int32_t n, double *xy, uint8_t *ok) {
    const int rc = ck_camera_check(cam);
    if (rc != CK_OK) return rc;
    if (!px || !xy || !ok || n < 0) return CK_EINVAL;
    double k[9];
    ckm_effective(cam->model, cam->k, k);
    for (int32_t i = 0; i < n; i++) {
        const int good = cam->model == CK_CAMERA_OPENCV5 ? ckm_opencv5_undistort(k, px[2 * i], px[2 * i + 1], xy + 2 * (size_t)i, xy + 2 * (size_t)i + 1)
                                                         : ckm_eucm_normalize(k, px[2 * i], px[2 * i + 1], xy + 2 * (size_t)i, xy + 2 * (size_t)i + 1);
        ok[i] = good ? 1 : 0;
    }
    return CK_OK;
}

int ck_camera_project_host(const ck_camera_t *cam, const double *xyz, int32_t n, double *px, uint8_t *ok) {
    const int rc = ck_camera_check(cam);
    if (rc != CK_OK) return rc;
    if (!xyz || !px || !ok || n < 0) return CK_EINVAL;
    double k[9];
    ckm_effective(cam->model, cam->k, k);
    for (int32_t i = 0; i < n; i++) {
        const double X = xyz[3 * (size_t)i], Y = xyz[3 * (size_t)i + 1], Z = xyz[3 * (size_t)i + 2];
        const int good = cam->model == CK_CAMERA_OPENCV5 ? ckm_opencv5_project(k, X, Y, Z, px + 2 * (size_t)i, px + 2 * (size_t)i + 1)
                                                         : ckm_eucm_project(k, X, Y, Z, px + 2 * (size_t)i, px + 2 * (size_t)i + 1);
        ok[i] = good ? 1 : 0;
    }
    return CK_OK;
}
