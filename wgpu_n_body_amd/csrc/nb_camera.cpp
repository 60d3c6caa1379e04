// nb_camera.cpp -- the host side of the renderer (include/nbody.h "Renderer"): the reference's camera
// (`Camera`, src/runners/online_renderer.rs:12-54) and the checks nb_sim_render makes before it
// touches a device.  The matrix is evaluated in double and rounded to float once; the drawing rule
// itself (nb_render.hip) takes the 16 floats and never depends on the host's libm.
#include <cmath>

#include "nb_common.hpp"
#include "nb_sim.hpp"

namespace {

constexpr uint32_t kMaxSide = 16384;

struct V3 {
    double x, y, z;
};
V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
V3 normalize(V3 a) {
    const double l = std::sqrt(dot(a, a));
    return {a.x / l, a.y / l, a.z / l};
}

bool size_ok(const char *what, uint32_t width, uint32_t height) {
    if (width >= 1 && width <= kMaxSide && height >= 1 && height <= kMaxSide) return true;
    nb::set_error("%s: width and height must be 1..%u (got %u x %u)", what, kMaxSide, width, height);
    return false;
}

}  // namespace

namespace nb {

int render_check_params(const nb_render_params *p) {
    if (!p) {
        set_error("render: params is null");
        return NB_ERR_INVALID;
    }
    if (!size_ok("render", p->width, p->height)) return NB_ERR_INVALID;
    if (p->flags & ~NB_RENDER_SRGB) {
        set_error("render: unknown flag bits 0x%x", p->flags & ~NB_RENDER_SRGB);
        return NB_ERR_INVALID;
    }
    if (!(p->alpha >= 0.f && p->alpha <= 1.f)) {
        set_error("render: alpha must be in [0, 1] (got %g)", (double)p->alpha);
        return NB_ERR_INVALID;
    }
    for (int k = 0; k < 3; ++k)
        if (!(p->clear[k] >= 0.f && p->clear[k] <= 1.f)) {
            set_error("render: clear[%d] must be in [0, 1] (got %g)", k, (double)p->clear[k]);
            return NB_ERR_INVALID;
        }
    if (!std::isfinite(p->half_size)) {
        set_error("render: half_size is not finite");
        return NB_ERR_INVALID;
    }
    for (int k = 0; k < 16; ++k)
        if (!std::isfinite(p->view_proj[k])) {
            set_error("render: view_proj[%d] is not finite", k);
            return NB_ERR_INVALID;
        }
    return NB_OK;
}

}  // namespace nb

extern "C" {

int nb_camera_default(nb_camera *cam, uint32_t width, uint32_t height) {
    if (!cam) {
        nb::set_error("camera_default: cam is null");
        return NB_ERR_INVALID;
    }
    if (!size_ok("camera_default", width, height)) return NB_ERR_INVALID;
    *cam = nb_camera{{0.f, 1.f, 2.f}, {0.f, 0.f, 0.f}, {0.f, 1.f, 0.f}, (float)width / (float)height,
                     45.f,            0.00001f,        100.f};  // online_renderer.rs:231-239
    return NB_OK;
}

int nb_camera_view_proj(const nb_camera *cam, float out[16]) {
    if (!cam || !out) {
        nb::set_error("camera_view_proj: null argument");
        return NB_ERR_INVALID;
    }
    const V3 eye{cam->eye[0], cam->eye[1], cam->eye[2]}, target{cam->target[0], cam->target[1], cam->target[2]},
        up{cam->up[0], cam->up[1], cam->up[2]};
    // cgmath Matrix4::look_at_rh = look_to_rh(eye, target - eye, up)
    const V3 f = normalize(sub(target, eye)), s = normalize(cross(f, up)), u = cross(s, f);
    const double view[4][4] = {{s.x, s.y, s.z, -dot(s, eye)},  // [row][column]
                               {u.x, u.y, u.z, -dot(u, eye)},
                               {-f.x, -f.y, -f.z, dot(f, eye)},
                               {0.0, 0.0, 0.0, 1.0}};
    // cgmath::perspective(Deg(fovy), aspect, near, far)
    const double aspect = cam->aspect, znear = cam->znear, zfar = cam->zfar;
    const double c = 1.0 / std::tan((double)cam->fovy_deg * (3.14159265358979323846 / 180.0) / 2.0);
    const double proj[4][4] = {{c / aspect, 0.0, 0.0, 0.0},
                               {0.0, c, 0.0, 0.0},
                               {0.0, 0.0, (zfar + znear) / (znear - zfar), 2.0 * zfar * znear / (znear - zfar)},
                               {0.0, 0.0, -1.0, 0.0}};
    // OPENGL_TO_WGPU_MATRIX (online_renderer.rs:41-46): z' = z / 2 + w / 2
    const double gl2wgpu[4][4] = {{1.0, 0.0, 0.0, 0.0}, {0.0, 1.0, 0.0, 0.0}, {0.0, 0.0, 0.5, 0.5}, {0.0, 0.0, 0.0, 1.0}};
    double pv[4][4];
    for (int r = 0; r < 4; ++r)
        for (int col = 0; col < 4; ++col) {
            double a = 0.0;
            for (int k = 0; k < 4; ++k) a += proj[r][k] * view[k][col];
            pv[r][col] = a;
        }
    float res[16];
    for (int r = 0; r < 4; ++r)
        for (int col = 0; col < 4; ++col) {
            double a = 0.0;
            for (int k = 0; k < 4; ++k) a += gl2wgpu[r][k] * pv[k][col];
            res[4 * col + r] = (float)a;
            if (!std::isfinite(res[4 * col + r])) {
                nb::set_error("camera_view_proj: the camera has no finite matrix (element [%d,%d])", r, col);
                return NB_ERR_INVALID;
            }
        }
    for (int k = 0; k < 16; ++k) out[k] = res[k];
    return NB_OK;
}

int nb_render_params_default(nb_render_params *params, uint32_t width, uint32_t height) {
    if (!params) {
        nb::set_error("render_params_default: params is null");
        return NB_ERR_INVALID;
    }
    nb_camera cam;
    if (int rc = nb_camera_default(&cam, width, height)) return rc;
    nb_render_params p{};
    p.width = width;
    p.height = height;
    if (int rc = nb_camera_view_proj(&cam, p.view_proj)) return rc;
    p.half_size = 0.006f;                             // online_renderer.rs:224
    p.clear[0] = 0.01f, p.clear[1] = 0.f, p.clear[2] = 0.05f;  // online_renderer.rs:345-349
    p.alpha = 0.25f;                                  // draw.wgsl:21
    p.flags = NB_RENDER_SRGB;
    *params = p;
    return NB_OK;
}

}  // extern "C"
