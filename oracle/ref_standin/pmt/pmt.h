/* Stand-in for pmt: interned symbols and long integers, nothing else. */
#ifndef REF_STANDIN_PMT_H
#define REF_STANDIN_PMT_H
#include <memory>
#include <string>

namespace pmt {
  struct pmt_base {
    bool is_symbol;
    std::string name;
    long number;
  };
  typedef std::shared_ptr<pmt_base> pmt_t;

  inline pmt_t string_to_symbol(const std::string &s) { return pmt_t(new pmt_base{true, s, 0}); }
  inline pmt_t intern(const std::string &s) { return string_to_symbol(s); }
  inline std::string symbol_to_string(const pmt_t &p) { return p->name; }
  inline pmt_t from_long(long v) { return pmt_t(new pmt_base{false, std::string(), v}); }
  inline long to_long(const pmt_t &p) { return p->number; }
  /* two symbols are the same object in pmt; here: the same name */
  inline bool eq(const pmt_t &a, const pmt_t &b)
  {
    if (!a || !b) return a == b;
    return a->is_symbol == b->is_symbol && (a->is_symbol ? a->name == b->name : a->number == b->number);
  }
  /* eqv: eq, and numbers of the same type with the same value; symbols and longs are all there is here, so the two coincide */
  inline bool eqv(const pmt_t &a, const pmt_t &b) { return eq(a, b); }
}
#endif
