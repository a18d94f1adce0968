// tgnh_receivers.h -- the table of receiving slots that the library's forces share (tgnh_virtual_sites.*, tgnh_drude_force.*,
// tgnh_bonded.*, tgnh_nonbonded.*'s evaluated exceptions): a force whose terms each push on a few slots is computed with one lane per
// RECEIVING slot, over the term table inverted on the host at set time.  Here: the kernels' view of the inverse, and the inversion.
// Its owner on the handle is tgnh_context.h's Receivers; what a lane does with it is tgnh_receiver_device.h's.  Read by host units
// and .hip units; no header the step kernels' unit reads changes with it.
#ifndef TGNH_RECEIVERS_H_
#define TGNH_RECEIVERS_H_

#include <algorithm>
#include <vector>

namespace tgnh {

// The inverse as the kernels read it: the slots that receive a share of some term, ascending, each with its list of (term, which
// of the term's particles the slot is) in CSR form, in ascending term order.  What a term and a role are is the feature's business.
struct ReceiverTable {
    const int* slot;                // [n]
    const int* start;               // [n + 1] into the two arrays below
    const int* term;                // [entries]
    const unsigned char* role;      // [entries]
    int n;                          // (every slot is a slot of the bound arrays, every term a row of its table: the host checked at set time)
};
inline bool receivers_ok(const ReceiverTable& t) { return t.n >= 1 && t.slot && t.start && t.term && t.role; }

// One share: `slot` receives from `term`, as the term's particle number `role`.  A setter pushes them in term order.
struct Share { int slot, term; unsigned char role; };
struct ReceiverLists {              // ReceiverTable's arrays on the host
    std::vector<int> slot, start, term;
    std::vector<unsigned char> role;
};
// The sort is stable, so a slot's entries keep the ascending term order they were pushed in.  That is the order a lane walks them
// in: the integer shares would sum to the same in any order, but where an energy is asked for a thread adds its terms' doubles in
// this order, which is part of the contract that the same table gives the same bits.
inline ReceiverLists invert_shares(std::vector<Share> shares) {
    std::stable_sort(shares.begin(), shares.end(), [](const Share& x, const Share& y) { return x.slot < y.slot; });
    ReceiverLists l;
    l.term.resize(shares.size());
    l.role.resize(shares.size());
    for (size_t e = 0; e < shares.size(); e++) {
        if (l.slot.empty() || l.slot.back() != shares[e].slot) { l.slot.push_back(shares[e].slot); l.start.push_back((int)e); }
        l.term[e] = shares[e].term;
        l.role[e] = shares[e].role;
    }
    l.start.push_back((int)shares.size());
    return l;
}

}  // namespace tgnh

#endif
