/* dvbt_map_impl.h -- HIP-backed body of gr::dvbt::dvbt_map (replaces lib/dvbt_map_impl.h of gr-dvbt; see hip_shell.h) */
#ifndef INCLUDED_DVBT_DVBT_MAP_IMPL_HIP_H
#define INCLUDED_DVBT_DVBT_MAP_IMPL_HIP_H

#include <dvbt/dvbt_map.h>
#include "hip_shell.h"

namespace gr {
  namespace dvbt {

    class dvbt_map_impl : public dvbt_map
    {
      DVBT_HIP_SHELL_MEMBERS(map)
    public:
      dvbt_map_impl(int nsize, dvbt_constellation_t constellation, dvbt_hierarchy_t hierarchy, dvbt_transmission_mode_t transmission, float gain);
      ~dvbt_map_impl() {}
    };

  } // namespace dvbt
} // namespace gr

#endif
