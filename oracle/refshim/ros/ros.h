// Stand-in for <ros/ros.h> (TEST INFRASTRUCTURE ONLY; see ../Eigen/Dense).
// NodeHandle::getParam is served from a process-wide map of strings that the driver fills (a
// leading '/' of the key is dropped, so "/q0" and "des_vel" address the same flat namespace).
// Values convert as roscpp converts an XmlRpc number: parsed as a double (or an int) and then
// cast to the requested type. advertise / publish do nothing; ROS_INFO / ROS_ERROR expand to
// nothing.
//
// F110_REFSHIM_GLOBAL_MATH_H: include <math.h> as well as <cmath>. With libstdc++ that header
// puts the float overloads of cos / sin into the global namespace, which decides what the
// reference's unqualified cos(float) in Constraints::FindHalfSpaces calls. Whether the real
// roscpp / Eigen include chain does so cannot be established without those headers; the driver
// is therefore built both ways (oracle/Makefile).
#ifndef F110_REFSHIM_ROS_H
#define F110_REFSHIM_ROS_H

#include <cmath>
#ifdef F110_REFSHIM_GLOBAL_MATH_H
#include <math.h>
#endif
#include <cstdlib>
#include <iostream>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#define ROS_INFO(...) ((void)0)
#define ROS_ERROR(...) ((void)0)
#define ROS_WARN(...) ((void)0)

namespace ros {

struct Time {
  Time() {}
  static Time now() { return Time(); }
};

class Publisher {
 public:
  template <typename M> void publish(const M&) const {}
};

inline std::map<std::string, std::string>& refshim_params() {
  static std::map<std::string, std::string> p;
  return p;
}

class NodeHandle {
 public:
  NodeHandle() {}
  template <typename M> Publisher advertise(const std::string&, int) { return Publisher(); }
  bool getParam(const std::string& key, double& v) const {
    const std::string* s = find(key);
    if (s) v = std::strtod(s->c_str(), nullptr);
    return s != nullptr;
  }
  bool getParam(const std::string& key, float& v) const {
    double d;
    if (!getParam(key, d)) return false;
    v = (float)d;
    return true;
  }
  bool getParam(const std::string& key, int& v) const {
    const std::string* s = find(key);
    if (s) v = (int)std::strtol(s->c_str(), nullptr, 10);
    return s != nullptr;
  }
  bool getParam(const std::string& key, std::string& v) const {
    const std::string* s = find(key);
    if (s) v = *s;
    return s != nullptr;
  }

 private:
  static const std::string* find(const std::string& key) {
    const std::string k = (!key.empty() && key[0] == '/') ? key.substr(1) : key;
    auto it = refshim_params().find(k);
    return it == refshim_params().end() ? nullptr : &it->second;
  }
};

}  // namespace ros

#endif
