// ray_demo -- ray casts through the adapter, for tests/test_gpu_adapter_rays.py.  A cube carrying a downward fan of rays
// (attached to it: given in its frame, never seeing its own hull) falls from z = 1.5 towards a ball (r = 0.15) right
// under it, a log lying along y at x = 0.45 and a cube at x = -0.45 (the adapter's plate: every box is the 0.3 cube),
// all three resting 1 mm in the ground.  60 x Step(5e-3): the carrier does not arrive, so its R stays the identity and
// the readings have closed forms at every step, from the Body objects the step pulled:
//   the ray from its centre straight down      t = (z_carrier - z_ball) - r      above the ball's pole
//   the ray 0.6 to its side straight down      t = z_carrier                     above the ground (also before any Step)
//   the rays from over the log and the cube    t = z_carrier - (z + r), z_carrier - (z + 0.15)
// The first two are checked to 1e-12, the last two to 1e-9; the level ray misses.  After every step the same poses in a
// scene that never stepped go through the stateless entry and must give the same bits as the device world's table.
// Then two such scenes, the carriers at different heights, as an EnsembleGroup: one table, one launch, each member's
// readings its own closed forms.  One JSON line; exit status 1 if any reading disagrees.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "eggshell_api.h"

namespace {

const double kDt = 5e-3, kBall = 0.15, kLogR = 0.1, kLogLen = 0.6;
const int kCarrier = 0, kBallBody = 1, kLogBody = 2, kCubeBody = 3;

class Scene : public Ensemble {
 public:
  void Add(const Body &b) { components_.push_back(std::make_shared<Body>(b)); n_ = (int)components_.size(); }
  void Setup() {
    Init();
    solver_params.method = EGS_SOR;
    solver_params.omega = 1.5;
    solver_params.max_iters = 500;
    solver_params.tol = 1e-9;
    solver_params.check_every = 1;
    cfm_coeff = 0.01;
  }
};

void Build(Scene *s, double z_carrier) {
  s->Add(Body(Vector3d(0, 0, z_carrier), Vector3d::Zero(), Matrix3d::Identity(), Vector3d::Zero()));
  s->Add(Body::Sphere(Vector3d(0, 0, kBall - 1e-3), Vector3d::Zero(), kBall));
  Body log = Body::Capsule(Vector3d(0.45, 0, kLogR - 1e-3), Vector3d::Zero(), kLogR, kLogLen);
  Matrix3d R = Matrix3d::Identity();   // the capsule's axis (the body's z) turned onto the world's y
  R(1, 1) = 0; R(1, 2) = 1; R(2, 1) = -1; R(2, 2) = 0;
  log.SetR(R);
  s->Add(log);
  s->Add(Body(Vector3d(-0.45, 0, 0.149), Vector3d::Zero(), Matrix3d::Identity(), Vector3d::Zero()));
}

// the fan, in the carrier's frame: down from the centre, from 0.6 to the side in y, from over the log and from over the
// cube, and one level ray
std::vector<Ray> Fan() {
  const Vector3d o[5] = {Vector3d(0, 0, 0), Vector3d(0, 0.6, 0), Vector3d(0.45, 0, 0), Vector3d(-0.45, 0, 0), Vector3d(0, 0, 0)};
  const Vector3d d[5] = {Vector3d(0, 0, -1), Vector3d(0, 0, -1), Vector3d(0, 0, -1), Vector3d(0, 0, -1), Vector3d(1, 0, 0)};
  std::vector<Ray> fan;
  for (int k = 0; k < 5; ++k) {
    Ray r;
    r.origin = o[k]; r.dir = d[k]; r.body = kCarrier;
    fan.push_back(r);
  }
  return fan;
}

int failures = 0;

void expect(bool ok, const char *what, int step) {
  if (ok) return;
  ++failures;
  std::fprintf(stderr, "ray_demo: %s at step %d\n", what, step);
}

// the closed forms on one scene's readings
void check(const Scene &s, const std::vector<RayHit> &h, int step) {
  const double zc = s.components()[kCarrier]->p()[2], zb = s.components()[kBallBody]->p()[2];
  expect(h[0].body == kBallBody && std::fabs(h[0].t - ((zc - zb) - kBall)) <= 1e-12, "the reading above the ball's pole", step);
  expect(std::fabs(h[0].normal[2] - 1.0) <= 1e-12 && std::fabs(h[0].point[2] - (zb + kBall)) <= 1e-12, "the pole's normal and point", step);
  expect(h[1].body == -1 && std::fabs(h[1].t - zc) <= 1e-12 && h[1].normal[2] == 1.0, "the reading above the ground", step);
  // the log's crest and the cube's top face, to 1e-9: a resting body may have crept sideways or tilted by that much
  const double zl = s.components()[kLogBody]->p()[2], zq = s.components()[kCubeBody]->p()[2];
  expect(h[2].body == kLogBody && std::fabs(h[2].t - (zc - (zl + kLogR))) <= 1e-9, "the reading above the log's crest", step);
  expect(h[3].body == kCubeBody && std::fabs(h[3].t - (zc - (zq + 0.15))) <= 1e-9, "the reading above the cube's top", step);
  expect(h[4].body == -2 && std::isinf(h[4].t) && h[4].normal.norm() == 0.0, "the level ray's miss", step);
}

bool same(const std::vector<RayHit> &a, const std::vector<RayHit> &b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i) {
    const double x[4] = {a[i].t, a[i].normal[0], a[i].normal[1], a[i].normal[2]};
    const double y[4] = {b[i].t, b[i].normal[0], b[i].normal[1], b[i].normal[2]};
    if (a[i].body != b[i].body || std::memcmp(x, y, sizeof x) != 0) return false;   // bits: -0.0 is not 0.0
  }
  return true;
}

// the same poses in a scene that never stepped: the stateless entry
std::vector<RayHit> Stateless(const Scene &s, const std::vector<Ray> &fan) {
  Scene probe;
  for (const auto &c : s.components()) probe.Add(*c);
  return probe.CastRays(fan);
}

}  // namespace

int main() {
  try {
    const std::vector<Ray> fan = Fan();
    const int steps = 60;
    Scene s;
    Build(&s, 1.5);
    s.Setup();
    std::vector<RayHit> h = s.CastRays(fan);   // before any Step: the stateless entry on the Body objects
    check(s, h, 0);
    expect(h[1].t == 1.5, "the height above the ground at the start", 0);
    std::printf("{\"steps\": %d, \"readings\": [", steps);
    for (int k = 1; k <= steps; ++k) {
      s.Step(kDt);
      h = s.CastRays(fan);                     // the device world's table against the state it holds
      check(s, h, k);
      expect(same(h, Stateless(s, fan)), "world and stateless readings differ", k);
      std::printf("%s[%.17g, %.17g, %.17g, %.17g, %.17g]", k > 1 ? ", " : "", s.components()[kCarrier]->p()[2], h[0].t, h[1].t, h[2].t,
                  h[3].t);
    }
    const RayHit one = s.CastRay(Vector3d(0.45, 0, 2.0), Vector3d(0, 0, -2.0));   // world frame, |d| = 2: t in units of d
    expect(one.body == kLogBody && std::fabs(one.t - (2.0 - (s.components()[kLogBody]->p()[2] + kLogR)) / 2.0) <= 1e-9,
           "the single ray onto the log's crest", steps);
    Scene a, b;
    Build(&a, 1.2); Build(&b, 1.8);
    a.Setup(); b.Setup();
    EnsembleGroup group({&a, &b});
    std::vector<std::vector<RayHit>> g;
    for (int k = 1; k <= 10; ++k) {
      group.Step(std::vector<double>{kDt, k == 5 ? 0.0 : kDt});   // b sits the fifth step out
      g = group.CastRays({fan, fan});
      check(a, g[0], 100 + k);
      check(b, g[1], 200 + k);
      expect(same(g[0], Stateless(a, fan)) && same(g[1], Stateless(b, fan)), "group and stateless readings differ", k);
    }
    std::printf("], \"group\": [%.17g, %.17g, %.17g, %.17g], \"single\": %.17g, \"failures\": %d}\n", a.components()[kCarrier]->p()[2],
                g[0][1].t, b.components()[kCarrier]->p()[2], g[1][1].t, one.t, failures);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "ray_demo: %s\n", e.what());
    return 1;
  }
  return failures ? 1 : 0;
}
