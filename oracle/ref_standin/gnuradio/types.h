/* Stand-in for GNU Radio's types.h: the item and vector typedefs the blocks name.
 * Also pulls in the standard headers that the real GNU Radio headers bring along
 * and that the block sources rely on without including them. */
#ifndef REF_STANDIN_GR_TYPES_H
#define REF_STANDIN_GR_TYPES_H
#include <cassert>
#include <cmath>
#include <complex>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

typedef std::complex<float> gr_complex;
typedef std::complex<double> gr_complexd;
typedef std::vector<int> gr_vector_int;
typedef std::vector<void *> gr_vector_void_star;
typedef std::vector<const void *> gr_vector_const_void_star;

/* there is no boost here: the blocks only name boost::shared_ptr */
namespace boost {
  template <class T> using shared_ptr = std::shared_ptr<T>;
}
#endif
