// tests/hostcheck/step_arith.cpp -- TEST HARNESS, not product code.
// The step's cheaper primitives of 2048_q-learning_amd/csrc/q2048_core.hpp (draws_prepare / draws_at, the integer
// epsilon threshold, the reward chain read through a LutImage) next to the definitions they must equal, compiled
// for the host so that tests/test_step_arithmetic.py can compare them bit for bit.
#include "q2048_core5.hpp"

using namespace q2048;

static const LutImage g_image = Q2048_LUT_IMAGE;

extern "C" {

void sa_draws(uint64_t seed, uint64_t env_id, uint32_t ctr, uint32_t stream, uint32_t* out) {
  const Draws d = draws(seed, env_id, ctr, stream);
  out[0] = d.x0; out[1] = d.x1; out[2] = d.x2; out[3] = d.x3;
}
// one prepare, then every counter of `ctr[0..n)`: the way a rollout loop uses the pair
void sa_draws_split(uint64_t seed, uint64_t env_id, const uint32_t* ctr, int64_t n, uint32_t stream, uint32_t* out) {
  const DrawPrep p = draws_prepare(seed, env_id, stream);
  for (int64_t i = 0; i < n; ++i) {
    const Draws d = draws_at(p, ctr[i]);
    out[4 * i] = d.x0; out[4 * i + 1] = d.x1; out[4 * i + 2] = d.x2; out[4 * i + 3] = d.x3;
  }
}

uint64_t sa_eps_threshold(double eps) { return eps_threshold(eps); }
int sa_draw_below(uint32_t x, uint64_t threshold) { return draw_below(x, threshold); }
int sa_eps_test_f64(uint32_t x, double eps) { return draw_uniform(x) < eps; }
// (action, explored) of both forms of choose_action
void sa_eps_greedy(double eps, uint32_t x_eps, uint32_t x_act, const float* q, int* out) {
  bool e0, e1;
  out[0] = eps_greedy(eps, x_eps, x_act, q[0], q[1], q[2], q[3], e0);
  out[1] = e0;
  out[2] = eps_greedy_at(eps_threshold(eps), x_eps, x_act, q[0], q[1], q[2], q[3], e1);
  out[3] = e1;
}

int sa_lut_image(double* out) {
  const double* p = reinterpret_cast<const double*>(&g_image);
  for (int i = 0; i < kLutImageDoubles; ++i) out[i] = p[i];
  return kLutImageDoubles;
}
// calculate_reward through the constexpr arrays (image = 0) or the image; prev is updated in place
double sa_reward(uint32_t score, int valid, int over, uint32_t L, uint8_t* prev, int image) {
  return image ? calculate_reward(score, valid != 0, over != 0, L, *prev, ImageLuts{&g_image})
               : calculate_reward(score, valid != 0, over != 0, L, *prev);
}
double sa_normalize(double r, int image) {
  return image ? normalize_reward(r, ImageLuts{&g_image}) : normalize_reward(r);
}
double sa_stall(uint32_t k, int image) { return image ? ImageLuts{&g_image}.stall(k) : lut_stall(k); }

}  // extern "C"
