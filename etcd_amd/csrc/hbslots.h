// hbslots.h — the role-ordered slot map of libhbnode (HBN_PLACE_ROLE).
//
// Plain C++ bookkeeping, no HIP and no engine types, so it is tested on the CPU
// alone (tests/asan/slots_asan.cpp).
//
// Layout after every re-pack (plan()), with nl led and no other live groups:
//
//     [0, nl)          the led groups (state == leader), dense
//     [nl, nl + no)    every other live group, dense
//     [nl + no, cap)   free
//
// Two adjacent ranges growing from slot 0: at most the one 64-slot tile that
// holds slot nl has groups of both kinds, and the live groups stay packed at
// the bottom of the slot space whatever the capacity is.
//
// Between re-packs the map only records what happened: a new group takes the
// slot above the other range (or, when the slot space is used up to the
// capacity, a hole a removal left), a removal leaves a hole, a role change
// leaves the group where it is.  Each of these marks its slot dirty.  plan()
// then looks at the dirty slots and at the two zones the range boundaries
// moved over, nothing else, and emits one move list with read-before-write
// semantics (hb_move_groups): every led group outside [0, nl) goes to a slot
// of that range that holds no led group, every other group outside
// [nl, nl + no) to a slot of that range that holds no other group.  A slot that
// is neither dirty nor in a boundary zone held the right kind at the last
// re-pack and still does.  Per role change that is at most 2 moves (the group,
// and the one the boundary passes over), per removal at most 2 (a led group's
// hole and the boundary, or the top of the other range), so
//     moves <= 2 * (groups whose led / not-led role changed + groups removed).
// With no free slot the same list holds swaps and cycles; no scratch slot is
// needed.
#ifndef HBSLOTS_H_
#define HBSLOTS_H_

#include <algorithm>
#include <cstdint>
#include <vector>

namespace hbslots {

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint32_t TILE = 64;  // slots per 64-byte line of a [slot][G] byte column / per wave
enum : uint8_t { EMPTY = 0, OTHER = 1, LED = 2 };

struct Move {
  uint32_t src, dst;
};

class SlotMap {
 public:
  // every slot empty
  void init(uint32_t capacity) {
    cap_ = capacity;
    role_.assign(capacity, EMPTY);
    mark_.assign(capacity, 0);
    dirty_.clear();
    holes_.clear();
    lead_ = top_ = 0;
    n_led_ = n_oth_ = 0;
    all_dirty_ = false;
  }
  // take over an arbitrary occupancy (roles[slot] = EMPTY / OTHER / LED): the
  // next plan() looks at every slot, and may move up to all of the groups
  void adopt(const std::vector<uint8_t>& roles) {
    init((uint32_t)roles.size());
    for (uint32_t s = 0; s < cap_; ++s) {
      role_[s] = roles[s];
      if (roles[s] == LED) ++n_led_;
      else if (roles[s] == OTHER) ++n_oth_;
      if (roles[s] != EMPTY) top_ = s + 1;
    }
    for (uint32_t s = 0; s < top_; ++s)
      if (role_[s] == EMPTY) holes_.push_back(s);
    all_dirty_ = true;
  }

  uint32_t capacity() const { return cap_; }
  uint32_t led() const { return n_led_; }
  uint32_t other() const { return n_oth_; }
  uint32_t top() const { return top_; }
  uint8_t role(uint32_t slot) const { return role_[slot]; }

  // A slot for a new group, which is not led: the one above the other range,
  // else a hole.  NONE when every slot is taken.
  uint32_t alloc() {
    uint32_t s;
    if (top_ < cap_) {
      s = top_++;
    } else if (!holes_.empty()) {
      s = holes_.back();
      holes_.pop_back();
      touch(s);
    } else {
      return NONE;
    }
    role_[s] = OTHER;
    ++n_oth_;
    return s;
  }
  // the group in `slot` is gone
  void release(uint32_t slot) {
    if (slot >= cap_ || role_[slot] == EMPTY) return;
    if (role_[slot] == LED) --n_led_;
    else --n_oth_;
    role_[slot] = EMPTY;
    holes_.push_back(slot);
    touch(slot);
  }
  // the group in `slot` is (not) led now; a no-op when nothing changes
  void set_led(uint32_t slot, bool led) {
    if (slot >= cap_ || role_[slot] == EMPTY) return;
    const uint8_t r = led ? LED : OTHER;
    if (role_[slot] == r) return;
    if (led) ++n_led_, --n_oth_;
    else --n_led_, ++n_oth_;
    role_[slot] = r;
    touch(slot);
  }

  // The re-pack: the moves that restore the layout (src[] distinct, dst[]
  // distinct, all sources read before any destination is written), applied to
  // the map at once.  `out` is cleared first.
  void plan(std::vector<Move>& out) {
    out.clear();
    const uint32_t nl = n_led_, nt = n_led_ + n_oth_;
    if (all_dirty_) {
      for (uint32_t s = 0; s < top_; ++s) touch(s);
    } else {
      for (uint32_t s = std::min(lead_, nl); s < std::max(lead_, nl); ++s) touch(s);  // the led boundary moved
      for (uint32_t s = nt; s < top_; ++s) touch(s);                                   // above the new top
    }
    led_out_.clear();
    oth_out_.clear();
    led_hole_.clear();
    oth_hole_.clear();
    for (uint32_t s : dirty_) {
      mark_[s] = 0;
      const uint8_t r = role_[s];
      const bool in_a = s < nl, in_b = s >= nl && s < nt;
      if (r == LED && !in_a) led_out_.push_back(s);
      if (r == OTHER && !in_b) oth_out_.push_back(s);
      if (in_a && r != LED) led_hole_.push_back(s);
      if (in_b && r != OTHER) oth_hole_.push_back(s);
    }
    dirty_.clear();
    holes_.clear();
    all_dirty_ = false;
    // (equal by counting: [0, nl) has nl slots and nl led groups exist, likewise the other range)
    const size_t kl = std::min(led_out_.size(), led_hole_.size()), ko = std::min(oth_out_.size(), oth_hole_.size());
    std::sort(led_out_.begin(), led_out_.end());
    std::sort(led_hole_.begin(), led_hole_.end());
    std::sort(oth_out_.begin(), oth_out_.end());
    std::sort(oth_hole_.begin(), oth_hole_.end());
    out.reserve(kl + ko);
    for (size_t i = 0; i < kl; ++i) out.push_back(Move{led_out_[i], led_hole_[i]});
    for (size_t i = 0; i < ko; ++i) out.push_back(Move{oth_out_[i], oth_hole_[i]});
    for (const Move& m : out) role_[m.src] = EMPTY;
    for (size_t i = 0; i < kl; ++i) role_[led_hole_[i]] = LED;
    for (size_t i = 0; i < ko; ++i) role_[oth_hole_[i]] = OTHER;
    lead_ = nl;
    top_ = nt;
  }

  // 64-slot aligned tiles that hold groups of both kinds (a scan: for statistics and tests)
  uint32_t mixed_tiles() const {
    uint32_t k = 0;
    for (uint32_t t = 0; t < top_; t += TILE) {
      bool led = false, oth = false;
      for (uint32_t s = t; s < top_ && s < t + TILE; ++s) {
        led |= role_[s] == LED;
        oth |= role_[s] == OTHER;
      }
      k += led && oth;
    }
    return k;
  }

 private:
  void touch(uint32_t s) {
    if (mark_[s]) return;
    mark_[s] = 1;
    dirty_.push_back(s);
  }
  uint32_t cap_ = 0;
  std::vector<uint8_t> role_, mark_;
  std::vector<uint32_t> dirty_, holes_;
  uint32_t lead_ = 0, top_ = 0;  // as the last re-pack left them: led = [0, lead_), top_ grows with alloc()
  uint32_t n_led_ = 0, n_oth_ = 0;
  bool all_dirty_ = false;
  std::vector<uint32_t> led_out_, oth_out_, led_hole_, oth_hole_;
};

}  // namespace hbslots
#endif  // HBSLOTS_H_
