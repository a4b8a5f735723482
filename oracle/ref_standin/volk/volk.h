/* Stand-in for VOLK: the generic definition of the one kernel the demapper calls
 * (third-party arithmetic, restated), and a fixed alignment. */
#ifndef REF_STANDIN_VOLK_H
#define REF_STANDIN_VOLK_H
#include <complex>
#include <cstddef>
#include <cstdlib>

typedef std::complex<float> lv_32fc_t;

static inline size_t volk_get_alignment(void) { return 16; }

static inline void *volk_malloc(size_t size, size_t alignment)
{
  void *p = 0;
  return posix_memalign(&p, alignment, size) == 0 ? p : 0;
}
static inline void volk_free(void *p) { free(p); }

/* target[i] = (re - re_i)^2 + (im - im_i)^2, in float */
static inline void volk_32fc_x2_square_dist_32f_generic(float *target, const lv_32fc_t *src0, const lv_32fc_t *points, unsigned int num_points)
{
  for (unsigned int i = 0; i < num_points; i++) {
    float dr = src0->real() - points[i].real();
    float di = src0->imag() - points[i].imag();
    target[i] = dr * dr + di * di;
  }
}
#define volk_32fc_x2_square_dist_32f volk_32fc_x2_square_dist_32f_generic
#define volk_32fc_x2_square_dist_32f_a volk_32fc_x2_square_dist_32f_generic
#define volk_32fc_x2_square_dist_32f_u volk_32fc_x2_square_dist_32f_generic
#endif
