/* energy_dispersal_impl.h -- HIP-backed body of gr::dvbt::energy_dispersal (replaces lib/energy_dispersal_impl.h of gr-dvbt; see hip_shell.h) */
#ifndef INCLUDED_DVBT_ENERGY_DISPERSAL_IMPL_HIP_H
#define INCLUDED_DVBT_ENERGY_DISPERSAL_IMPL_HIP_H

#include <dvbt/energy_dispersal.h>
#include "hip_shell.h"

namespace gr {
  namespace dvbt {

    class energy_dispersal_impl : public energy_dispersal
    {
      DVBT_HIP_SHELL_MEMBERS(energy_dispersal)
    public:
      energy_dispersal_impl(int nsize);
      ~energy_dispersal_impl() {}
    };

  } // namespace dvbt
} // namespace gr

#endif
